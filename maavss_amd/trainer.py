"""Training step of the hot path: loss, backward, gradient all-reduce, Adam.

Mirrors the inner loop of the reference trainer (train_avse_frames.py:150-181):
    yh_stft, yh_attn, latent = model(x_stft, x_attn)
    loss = (mse(yh_stft, y_stft) + loss_coeff * mse(yh_attn, y_attn)) / num_seq ; loss.backward()
    optimizer.step(); optimizer.zero_grad()
with every tensor operation in libmaavss_hip.so.  Two entry levels:

* `FusedAdam`   -- drop-in for `torch.optim.Adam(model.parameters(), lr=...)` (train_avse_frames.py:92): all
                   parameters / gradients / moments live in flat f32 buffers and one HIP kernel updates them.
* `TrainStep`   -- the whole step without autograd: engine forward, fused MSE pair + gradients, hand-written
                   backward straight into the flat gradient buffer, RCCL all-reduce of the gradients
                   (one process per GPU, torch.distributed backend "nccl" = RCCL over xGMI) overlapped with
                   the encoder backward, fused Adam.  This is what bench.py times.

Data parallelism: clips are independent, the batch dimension is sharded across ranks, weights
are replicated (rank 0's parameters and BatchNorm buffers are broadcast when a TrainStep is built, as DDP
does); the only mandatory collective is the gradient sum.  BatchNorm uses per-rank batch statistics by default
(as torch DDP does without SyncBatchNorm); `TrainStep(sync_bn=True)` all-reduces the per-channel sums instead,
which reproduces the single-device reference on the concatenated batch -- documented in DESIGN.md.
"""
import math

import torch

from . import ops
from .spectral_loss import SpectralLoss
from .wave_loss import WaveformLoss

_FUSION_PREFIXES = ("lstm.", "fc1.", "fc2.", "a_fc1.", "v_fc1.")


def _align(n, a=64):
    return (n + a - 1) // a * a


class FlatParams:
    """Re-homes the parameters of a module in one flat f32 buffer (+ a flat gradient buffer).

    Layout: [fusion segment: lstm, fc1, fc2, heads | encoder segment: everything else], each tensor
    64-element aligned.  The fusion segment holds 98 % of the bytes and its gradients are complete first
    in the backward pass, so it is all-reduced while the conv backward still runs."""

    def __init__(self, model):
        named = [(n, p) for n, p in model.named_parameters() if not n.startswith("stft_autoencoder.")]
        fusion = [(n, p) for n, p in named if n.startswith(_FUSION_PREFIXES)]
        other = [(n, p) for n, p in named if not n.startswith(_FUSION_PREFIXES)]
        self.names, self.offsets, self.shapes = [], {}, {}
        self.torch_order = [n for n, _ in named]     # index i of torch.optim.Adam(model.parameters()).state_dict()
        off = 0
        for n, p in fusion + other:
            self.names.append(n)
            self.offsets[n] = off
            self.shapes[n] = tuple(p.shape)
            off = _align(off + p.numel())
            if n == fusion[-1][0]:
                self.fusion_end = off
        self.total = off
        dev = named[0][1].device
        self.params = torch.zeros(self.total, device=dev, dtype=torch.float32)
        self.grads = torch.zeros(self.total, device=dev, dtype=torch.float32)
        self.param_views, self.grad_views, self.tensors = {}, {}, {}
        for n, p in fusion + other:
            o, k = self.offsets[n], p.numel()
            pv = self.params[o:o + k].view(p.shape)
            pv.copy_(p.data)
            p.data = pv
            gv = self.grads[o:o + k].view(p.shape)
            p.grad = gv
            self.param_views[n], self.grad_views[n], self.tensors[n] = pv, gv, p
        # names whose gradient was produced since the last zero_grad(): Adam skips the others, like torch.optim.Adam skips
        # parameters whose .grad is None (e.g. stft_decoder.* under forward(), frozen sub-networks)
        self.touched = set()
        model._maavss_flat = self

    def mark(self, names):
        self.touched.update(names)

    def check_links(self):
        """The model's parameters must still be the flat views (model.to() / .float() / zero_grad(set_to_none=True) after
        construction re-home them).  A detached .grad is folded back in (None = no gradient this step, a foreign tensor
        is copied); a re-homed parameter cannot be repaired silently and raises."""
        from ._lib import MaavssError
        for n, p in self.tensors.items():
            if p.data_ptr() != self.param_views[n].data_ptr():
                raise MaavssError(f"parameter {n} no longer lives in the flat buffer (model.to()/.float() after the optimizer "
                                  f"was built?): build FusedAdam / TrainStep after moving the model")
            gv = self.grad_views[n]
            if p.grad is None:
                self.touched.discard(n)
                p.grad = gv
            elif p.grad.data_ptr() != gv.data_ptr():
                gv.copy_(p.grad)
                p.grad = gv
                self.touched.add(n)


def _numel(shape):
    k = 1
    for d in shape:
        k *= d
    return k


def default_decay_filter(name, param):
    """The tensors AdamW's decay applies to by default: everything with two or more dimensions (conv and linear weights, the LSTM's
    weight_ih / weight_hh); biases and BatchNorm weight and bias are left out."""
    return param.ndim >= 2


def plan_launches(runs, flat, weight_decay, max_segments=None):
    """Pure planning of the maavss_adamw_ema_step launches: `runs` as FusedAdam._runs() gives them, `weight_decay` {name: float}.
    One decay-table segment per tensor (its 64-aligned extent); a run with more than `max_segments` (the table's capacity,
    ops.ADAMW_MAX_SEGMENTS) tensors is split into consecutive launches.  -> [dict(lo, hi, step, names, ends, wd)]: `ends` are the
    segment ends relative to `lo`, `hi` never passes flat.total."""
    cap = ops.ADAMW_MAX_SEGMENTS if max_segments is None else int(max_segments)
    if cap < 1:
        raise ValueError("max_segments must be >= 1")
    out = []
    for lo, hi, st, names in runs:
        for a in range(0, len(names), cap):
            part = names[a:a + cap]
            plo = flat.offsets[part[0]]
            ends = [_align(flat.offsets[n] + _numel(flat.shapes[n])) - plo for n in part]
            out.append(dict(lo=plo, hi=min(plo + ends[-1], flat.total), step=st, names=list(part), ends=ends,
                            wd=[float(weight_decay.get(n, 0.0)) for n in part]))
    return out


class _EmaWeights:
    """Context manager of FusedAdam.ema_weights(): two launches of the swap kernel, no synchronisation."""

    def __init__(self, opt):
        self.opt = opt

    def __enter__(self):
        from ._lib import MaavssError
        o = self.opt
        if o.ema is None:
            raise MaavssError("ema_weights(): this optimizer keeps no weight average (ema_decay=None)")
        if o._ema_swapped:
            raise MaavssError("ema_weights() is not re-entrant: the averaged weights are already in the parameter buffer")
        o.flat.check_links()
        ops.swap_f32(o.flat.params, o.ema)
        o._ema_swapped = True
        return o

    def __exit__(self, *exc):
        o = self.opt
        ops.swap_f32(o.flat.params, o.ema)
        o._ema_swapped = False
        return False


class FusedAdam:
    """torch.optim.Adam semantics (betas .9/.999, eps 1e-8, no weight decay, no amsgrad) in HIP launches over the flat
    buffers.  Like torch, a parameter is only stepped when a backward pass produced a gradient for it since the last
    zero_grad() (frozen sub-networks and stft_decoder.* under forward() are left alone, keep their moments and their
    own step count); contiguous runs of stepped parameters share one launch -- one launch in the usual case.

    `max_grad_norm` (None = off: the launches are exactly the ones above) clips the global 2-norm of the gradient the way
    `torch.nn.utils.clip_grad_norm_(params, max_grad_norm)` does before `optimizer.step()`, over exactly the parameters this step
    updates (touched and requires_grad, as torch clips those whose .grad is not None): one segmented reduction over the flat
    gradient buffer (tensor_stats.TensorStats) leaves the norm and the coefficient on the device and the Adam kernel reads the
    coefficient from there -- no host synchronisation.  Unlike torch, the gradients are NOT rescaled in memory: `flat.grads` keeps the
    unclipped values, the scale is applied inside the Adam kernel.  `grad_norm` (the norm of grad_scale * g) and `clip_scale`
    (grad_scale * min(1, max_grad_norm / (norm + 1e-6))) are the device scalars of the last step; a non-finite gradient makes them
    NaN (any NaN) or +inf / 0 (an inf, no NaN), as torch's error_if_nonfinite=False -- the caller decides when to look.

    Beyond the reference (all off by default: step() then issues exactly the launches above; with any of `weight_decay`, `ema_decay`,
    `skip_nonfinite` set, every run goes through maavss_adamw_ema_step instead -- one kernel that decays, steps and averages):

    * `weight_decay`, `decay_filter(name, param) -> bool`: torch.optim.AdamW's decoupled decay, p *= 1 - lr * weight_decay before the
      Adam update, on the tensors the filter accepts (default_decay_filter: ndim >= 2).  state_dict() reports the decay in torch's
      one-group layout and loads into torch.optim.AdamW; the filter is code and is not stored (torch would decay every tensor).
    * `ema_decay` d in [0, 1): a second flat buffer `ema` = d * ema + (1 - d) * p after every update, a copy of the weights when the
      optimizer is built and after ema_reset().  Only stepped runs update it: a frozen tensor's average stays equal to its weights.
      `ema_warmup`: update number t (from 0) uses min(d, (1 + t) / (10 + t)).  ema_state_dict() / load_ema_state_dict() and the
      ema_weights() context manager give access.  BatchNorm running statistics are buffers, not parameters: they are not averaged, and
      inside ema_weights() the model runs the averaged weights with the LIVE running statistics.
    * `skip_nonfinite`: a step whose gradient norm (grad_norm, from the same reduction clipping uses; with max_grad_norm=None it runs
      with max_norm = inf) is NaN or infinite leaves weights, moments and average untouched, decided on the device without a host
      synchronisation.  `skipped_steps` is a device int32 [1], read when the caller chooses.  Deviation from torch.cuda.amp.GradScaler:
      a skipped step still advances the host step counts, the average's update count and the schedule -- the bias correction moves on by
      one step while the moments do not move.
    * `lr` may be a maavss_amd.LRSchedule: every step() takes the next rate from it; `lr` / the param group's "lr" is then the rate
      of the last step."""

    def __init__(self, model_or_flat, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None, weight_decay=0.0, decay_filter=None,
                 ema_decay=None, ema_warmup=False, skip_nonfinite=False):
        from .schedule import LRSchedule
        self.flat = model_or_flat if isinstance(model_or_flat, FlatParams) else FlatParams(model_or_flat)
        self.schedule = lr if isinstance(lr, LRSchedule) else None
        if self.schedule is not None:
            lr = self.schedule.lr(self.schedule.t)
        self.lr, self.betas, self.eps = lr, betas, eps
        if max_grad_norm is not None and not float(max_grad_norm) >= 0.0:
            raise ValueError("max_grad_norm must be None or >= 0")
        if not 0.0 <= float(weight_decay) < float("inf"):
            raise ValueError("weight_decay must be finite and >= 0")
        if ema_decay is not None and not 0.0 <= float(ema_decay) < 1.0:
            raise ValueError("ema_decay must be None or in [0, 1)")
        self.weight_decay = float(weight_decay)
        self.decay_filter = default_decay_filter if decay_filter is None else decay_filter
        self._decayed = None                    # {name: the filter's answer}, asked once, when first needed
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.ema_warmup, self.skip_nonfinite = bool(ema_warmup), bool(skip_nonfinite)
        self.ema = None if ema_decay is None else self.flat.params.clone()
        self.ema_updates = 0
        self._ema_swapped = False
        self.skipped_steps = torch.zeros(1, dtype=torch.int32, device=self.flat.params.device) if skip_nonfinite else None
        self.max_grad_norm = max_grad_norm
        self.grad_stats = None                  # tensor_stats.TensorStats over flat.grads, built by the first clipped step
        self.grad_norm = self.clip_scale = None
        self.exp_avg = torch.zeros_like(self.flat.params)
        self.exp_avg_sq = torch.zeros_like(self.flat.params)
        self.steps = {n: 0 for n in self.flat.names}          # per-parameter step count (torch keeps one per parameter)

    @property
    def step_count(self):
        return max(self.steps.values())

    @step_count.setter
    def step_count(self, n):
        self.steps = {k: int(n) for k in self.steps}

    def _runs(self):
        """[(lo, hi, step, names)]: maximal runs of touched parameters with equal step counts, in buffer order.  Pure planning:
        the per-parameter step counts are committed by step() once the launches are issued."""
        f, runs = self.flat, []
        for n in f.names:
            if n not in f.touched or not f.tensors[n].requires_grad:
                continue
            lo, st = f.offsets[n], self.steps[n] + 1
            k = 1
            for d in f.shapes[n]:
                k *= d
            hi = _align(lo + k)
            if runs and runs[-1][1] == lo and runs[-1][2] == st:
                runs[-1][1] = hi
                runs[-1][3].append(n)
            else:
                runs.append([lo, hi, st, [n]])
        return [tuple(r) for r in runs]

    def _commit(self, runs):
        for _, _, st, names in runs:
            for n in names:
                self.steps[n] = st

    @property
    def decayed(self):
        """{parameter name: whether weight_decay applies to it} -- decay_filter(name, param) of every tensor of the layout."""
        if self._decayed is None:
            self._decayed = {n: bool(self.decay_filter(n, self.flat.tensors[n])) for n in self.flat.names}
        return self._decayed

    @property
    def extended(self):
        """True when step() goes through maavss_adamw_ema_step (any of weight decay, weight average, non-finite skip is on)."""
        return self.weight_decay != 0.0 or self.ema is not None or self.skip_nonfinite

    def _next_ema_decay(self):
        """The decay of average update number `ema_updates` (host arithmetic)."""
        t = self.ema_updates
        return min(self.ema_decay, (1.0 + t) / (10.0 + t)) if self.ema_warmup else self.ema_decay

    def _step_extended(self, runs, grad_scale):
        f = self.flat
        with_norm = self.max_grad_norm is not None or self.skip_nonfinite
        wd = {n: self.weight_decay for n in f.names if self.decayed[n]}
        launches = plan_launches(runs, f, wd)
        d = self._next_ema_decay() if self.ema is not None else 0.0
        for k, ln in enumerate(launches):
            lo, hi = ln["lo"], ln["hi"]
            ops.adamw_ema_step(f.params[lo:hi], f.grads[lo:hi], self.exp_avg[lo:hi], self.exp_avg_sq[lo:hi], self.lr, ln["step"],
                               ln["ends"], ln["wd"], ema=None if self.ema is None else self.ema[lo:hi], ema_decay=d, betas=self.betas,
                               eps=self.eps, grad_scale=grad_scale, scale_dev=self.clip_scale if with_norm else None,
                               norm_dev=self.grad_norm if self.skip_nonfinite else None, skipped=self.skipped_steps,
                               count_skip=self.skip_nonfinite and k == 0)
        if self.ema is not None and launches:
            self.ema_updates += 1

    def step(self, grad_scale=1.0):
        if self._ema_swapped:
            from ._lib import MaavssError
            raise MaavssError("step() inside ema_weights(): the parameter buffer holds the averaged weights")
        self.flat.check_links()
        runs = self._runs()
        if self.schedule is not None:
            self.lr = self.schedule.next_lr()
        extended = self.extended
        if (self.max_grad_norm is not None or self.skip_nonfinite) and runs:
            if self.grad_stats is None:
                from .tensor_stats import TensorStats
                self.grad_stats = TensorStats(self.flat, bins=1)
            # without clipping, max_norm = inf: the coefficient min(1, inf / (norm + 1e-6)) is 1 for every finite norm, scale = grad_scale
            out = self.grad_stats.run(self.flat.grads, names=[n for r in runs for n in r[3]], hist=False,
                                      max_norm=self.max_grad_norm if self.max_grad_norm is not None else float("inf"),
                                      grad_scale=grad_scale)
            self.grad_norm, self.clip_scale = out["norm"], out["scale"]
        if extended:
            self._step_extended(runs, grad_scale)
            self._commit(runs)
            return
        for lo, hi, st, _ in runs:
            hi = min(hi, self.flat.total)
            if self.max_grad_norm is not None:
                ops.adam_step_dscale(self.flat.params[lo:hi], self.flat.grads[lo:hi], self.exp_avg[lo:hi], self.exp_avg_sq[lo:hi],
                                     self.lr, st, self.clip_scale, self.betas, self.eps)
            else:
                ops.adam_step(self.flat.params[lo:hi], self.flat.grads[lo:hi], self.exp_avg[lo:hi], self.exp_avg_sq[lo:hi],
                              self.lr, st, self.betas, self.eps, grad_scale)
        self._commit(runs)

    def zero_grad(self, set_to_none=False):
        """memset of the flat gradient buffer; the views stay attached to p.grad whatever `set_to_none` says (gradients
        are accumulated in place).  Parameters count as gradient-less until the next backward produces one."""
        self.flat.check_links()
        self.flat.grads.zero_()
        self.flat.touched.clear()

    def state_dict(self):
        """torch.optim.Adam's layout (what utilities.save_checkpoint stores as 'optimizer_state_dict',
        utilities.py:168-175): per-parameter step / exp_avg / exp_avg_sq keyed by the position of the parameter in
        model.parameters(), plus one param_group.  Parameters that were never stepped have no entry, as in torch."""
        f = self.flat
        state = {}
        for i, n in enumerate(f.torch_order):
            if self.steps[n] == 0:
                continue
            o, k = f.offsets[n], 1
            for d in f.shapes[n]:
                k *= d
            state[i] = {"step": torch.tensor(float(self.steps[n])),
                        "exp_avg": self.exp_avg[o:o + k].view(f.shapes[n]).clone(),
                        "exp_avg_sq": self.exp_avg_sq[o:o + k].view(f.shapes[n]).clone()}
        group = {"lr": self.lr, "betas": tuple(self.betas), "eps": self.eps, "weight_decay": self.weight_decay if self.weight_decay else 0,
                 "amsgrad": False, "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                 "params": list(range(len(f.torch_order)))}
        if self.weight_decay:
            group["decoupled_weight_decay"] = True      # torch.optim.AdamW's marker: without it torch reads the decay as Adam's L2 term
        return {"state": state, "param_groups": [group]}

    def ema_reset(self):
        """The average starts over as a copy of the current weights (update count 0)."""
        from ._lib import MaavssError
        if self.ema is None:
            raise MaavssError("ema_reset(): this optimizer keeps no weight average (ema_decay=None)")
        if self._ema_swapped:
            raise MaavssError("ema_reset() inside ema_weights()")
        self.ema.copy_(self.flat.params)
        self.ema_updates = 0

    def ema_weights(self):
        """Context manager: inside the block the flat parameter buffer -- hence the model, Validator, Enhancer and model.state_dict()
        -- holds the averaged weights and `ema` holds the raw ones; they are swapped back on exit.  Two launches of
        maavss_swap_f32, no third buffer, no synchronisation.  BatchNorm running statistics are buffers and stay the live ones.
        Nesting the context and calling step() inside it raise."""
        return _EmaWeights(self)

    def ema_state_dict(self):
        """{parameter name: averaged tensor} in the keys of model.state_dict(), plus "num_updates"."""
        from ._lib import MaavssError
        if self.ema is None:
            raise MaavssError("ema_state_dict(): this optimizer keeps no weight average (ema_decay=None)")
        f = self.flat
        src = f.params if self._ema_swapped else self.ema
        sd = {n: src[f.offsets[n]:f.offsets[n] + _numel(f.shapes[n])].view(f.shapes[n]).clone() for n in f.torch_order}
        sd["num_updates"] = torch.tensor(self.ema_updates, dtype=torch.int64)
        return sd

    def load_ema_state_dict(self, sd):
        from ._lib import MaavssError
        if self.ema is None:
            raise MaavssError("load_ema_state_dict(): this optimizer keeps no weight average (ema_decay=None)")
        if self._ema_swapped:
            raise MaavssError("load_ema_state_dict() inside ema_weights()")
        f = self.flat
        for n in f.torch_order:
            if n not in sd:
                raise ValueError(f"averaged weights: no entry for parameter {n}")
            if tuple(sd[n].shape) != f.shapes[n]:
                raise ValueError(f"averaged weights of {n} have shape {tuple(sd[n].shape)}, expected {f.shapes[n]}")
        for n in f.torch_order:
            self.ema[f.offsets[n]:f.offsets[n] + _numel(f.shapes[n])].copy_(sd[n].reshape(-1))
        self.ema_updates = int(sd.get("num_updates", 0))

    def load_state_dict(self, sd):
        """Accepts the dict above and a reference checkpoint's torch.optim.Adam state (parameters the reference never
        stepped -- stft_decoder.* under forward() -- have no entry there: their moments and step count stay zero).  Like torch, the
        group's lr, betas, eps and weight_decay replace the constructor's (a torch.optim.AdamW state brings its decay along; a non-zero
        decay of plain torch.optim.Adam, the L2 form, is refused).  With a schedule, the next step takes its rate from the schedule again."""
        f = self.flat
        groups = sd["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(f.torch_order):
            raise ValueError(f"optimizer state has {sum(len(g['params']) for g in groups)} parameters in {len(groups)} group(s); "
                             f"this model has {len(f.torch_order)} in one")
        self.lr = float(groups[0]["lr"])
        self.betas = tuple(float(b) for b in groups[0]["betas"])
        self.eps = float(groups[0]["eps"])
        wd = float(groups[0].get("weight_decay", 0))
        if wd != 0.0 and not groups[0].get("decoupled_weight_decay", False):
            raise ValueError(f"optimizer state has weight_decay {wd} as torch.optim.Adam's L2 term; only AdamW's decoupled decay is implemented")
        self.weight_decay = wd
        self.exp_avg.zero_()
        self.exp_avg_sq.zero_()
        self.steps = {n: 0 for n in f.names}
        for i, n in enumerate(f.torch_order):
            st = sd["state"].get(i, sd["state"].get(str(i)))
            if st is None:
                continue
            o, k = f.offsets[n], st["exp_avg"].numel()
            if tuple(st["exp_avg"].shape) != f.shapes[n]:
                raise ValueError(f"optimizer state of parameter {i} ({n}) has shape {tuple(st['exp_avg'].shape)}, expected {f.shapes[n]}")
            self.exp_avg[o:o + k].copy_(st["exp_avg"].reshape(-1))
            self.exp_avg_sq[o:o + k].copy_(st["exp_avg_sq"].reshape(-1))
            self.steps[n] = int(float(st["step"]))


class GradSync:
    """Sum-all-reduce of the flat gradient buffer across data-parallel ranks (K18).

    Works on any torch.distributed backend ("nccl" = RCCL on ROCm for the GPUs, "gloo" in CPU tests); with world_size 1
    every method is a no-op.  The buffer is reduced in BUCKETS, in the order the backward pass completes them
    ("bucketed in reverse-layer order to overlap with conv3d backward"): with a FlatParams layout the fusion
    segment is one bucket per top-level module -- heads (a_fc1, v_fc1), fc2, fc1, lstm -- each launched asynchronously by
    `grad_ready(name)` the moment its last gradient has been enqueued, so the first all-reduce (the 26 M-float v_fc1 head)
    starts after the heads' weight gradients, not after the whole fusion segment; the encoder segment follows in `finish()`,
    which also waits for everything.  Only parameters that receive a gradient this step take part (`begin(expected)`, the
    same set on every rank): a bucket without any is skipped, stale regions inside a reduced bucket are zeroed first -- a
    frozen parameter's old gradient is never summed over the ranks step after step.
    `start_fusion()` (round-1/2 interface) launches whatever is left of the fusion segment in one go."""

    def __init__(self, grads, fusion_end, process_group=None, flat=None, wire_dtype=None):
        import torch.distributed as dist
        if wire_dtype not in (None, "f32", "bf16"):
            raise ValueError("wire_dtype must be None / 'f32' or 'bf16'")
        # "bf16": every bucket is rounded to bf16 for the collective (half the xGMI bytes; the sum over the ranks is then a bf16 sum)
        # and widened back into the f32 master buffer in finish().  Device tensors only: the conversion is a HIP kernel.
        self.wire_bf16 = wire_dtype == "bf16"
        self._wire = None
        self.dist = dist
        self.enabled = dist.is_available() and dist.is_initialized() and dist.get_world_size(process_group) > 1
        self.world = dist.get_world_size(process_group) if self.enabled else 1
        self.group = process_group
        self.grads, self.fusion_end = grads, fusion_end
        # buckets: [lo, hi) of the flat buffer + the (name, lo, hi) of the parameters inside, fusion segment first
        self.buckets = []
        if flat is not None:
            for n in flat.names:
                lo = flat.offsets[n]
                k = 1
                for d in flat.shapes[n]:
                    k *= d
                hi = _align(lo + k)
                key = "encoders" if lo >= fusion_end else n.split(".")[0]
                if self.buckets and self.buckets[-1]["key"] == key:
                    self.buckets[-1]["hi"] = hi
                    self.buckets[-1]["params"].append((n, lo, hi))
                else:
                    self.buckets.append(dict(key=key, lo=lo, hi=hi, params=[(n, lo, hi)]))
            self.buckets[-1]["hi"] = min(self.buckets[-1]["hi"], grads.numel())
        else:
            self.buckets = [dict(key="fusion", lo=0, hi=fusion_end, params=[]),
                            dict(key="encoders", lo=fusion_end, hi=grads.numel(), params=[])]
        self._bucket_of = {n: i for i, b in enumerate(self.buckets) for n, _, _ in b["params"]}
        self._expected, self._ready, self._launched, self._pending = None, set(), set(), []
        self.launch_log = []          # keys of the buckets in launch order, per step (tests, tracing)

    def broadcast(self, tensors, src=0):
        """Make the replicas identical: rank `src`'s values everywhere (parameters, BatchNorm buffers), as DDP does at
        construction.  No-op with one rank."""
        if self.enabled:
            for t in tensors:
                self.dist.broadcast(t, src=src, group=self.group)

    def sum_(self, t):
        """in-place sum of a small tensor over the ranks (global-batch BatchNorm sums)"""
        if self.enabled:
            self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM, group=self.group)
        return t

    def begin(self, expected=None):
        """Start of a backward pass whose gradients will be reduced: `expected` = names that will receive a gradient
        (None = every parameter).  Must be the same on every rank (it follows requires_grad, which is)."""
        self._expected = None if expected is None else set(expected)
        self._ready, self._launched, self._pending, self.launch_log = set(), set(), [], []

    def _wanted(self, b):
        return [p for p in b["params"] if self._expected is None or p[0] in self._expected]

    def _launch(self, i):
        if i in self._launched:
            return
        self._launched.add(i)
        b = self.buckets[i]
        if not self.enabled or b["hi"] <= b["lo"]:
            return
        if b["params"]:
            wanted = self._wanted(b)
            if not wanted:
                return                                   # nothing in this bucket received a gradient: not reduced at all
            if len(wanted) < len(b["params"]):
                keep = {p[0] for p in wanted}
                for n, lo, hi in b["params"]:
                    if n not in keep:
                        self.grads[lo:min(hi, b["hi"])].zero_()      # stale gradient of a frozen parameter
        self.launch_log.append(b["key"])
        if self.wire_bf16:
            if self._wire is None:
                self._wire = torch.empty(self.grads.numel(), device=self.grads.device, dtype=torch.bfloat16)
            lo, hi = b["lo"], (b["hi"] + 7) // 8 * 8
            hi = min(hi, self.grads.numel() // 8 * 8)
            ops.f32_to_bf16(self.grads[lo:hi], self._wire[lo:hi])
            work = self.dist.all_reduce(self._wire[lo:hi], op=self.dist.ReduceOp.SUM, group=self.group, async_op=True)
            self._pending.append((work, lo, hi))
            return
        self._pending.append((self.dist.all_reduce(self.grads[b["lo"]:b["hi"]], op=self.dist.ReduceOp.SUM, group=self.group,
                                                   async_op=True), None, None))

    def grad_ready(self, name):
        """The gradient of `name` has been enqueued on the current stream; launches its bucket when that completes it."""
        i = self._bucket_of.get(name)
        if i is None or self.buckets[i]["key"] == "encoders":
            return
        self._ready.add(name)
        if all(p[0] in self._ready for p in self._wanted(self.buckets[i])):
            self._launch(i)

    def start_fusion(self):
        for i, b in enumerate(self.buckets):
            if b["key"] != "encoders":
                self._launch(i)

    def finish(self):
        self.start_fusion()
        for i, b in enumerate(self.buckets):
            self._launch(i)
        for w, lo, hi in self._pending:
            w.wait()
            if lo is not None:
                ops.bf16_to_f32(self._wire[lo:hi], self.grads[lo:hi])
        self._pending = []
        self._expected, self._ready, self._launched = None, set(), set()


def shard_batch(global_batch, rank, world):
    """Contiguous shard [lo, hi) of the clip batch owned by `rank` (clips are independent units)."""
    base, rem = divmod(global_batch, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def sliding_windows(x_stft, y_stft, x_attn, y_attn, num_frames, hops_per_frame, num_seq):
    """The reference's window slicing (train_avse_frames.py:143-163) as views, shared by TrainStep.sliding_window_step and
    quality.Validator.add_clips: yields (j, x_a, x_v, y_a, y_v) for j < num_seq -- frames [j, j + num_frames) of x_attn [B,1,T,H,W] with
    the matching STFT frames of x_stft [B,2,T_a,F]; the targets are attention frame j + idx_mid of y_attn and the STFT frames of that
    video frame of y_stft, idx_mid = (num_seq - 1) // 2 (:105)."""
    hpf, ns = hops_per_frame, num_seq
    mid = (ns - 1) // 2
    assert x_attn.shape[2] >= num_frames + ns - 1 and x_stft.shape[2] >= hpf * (num_frames + ns - 1)
    for j in range(ns):
        xa = x_stft[:, :, hpf * j:hpf * (j + num_frames), :]
        ya = y_stft[:, :, hpf * (j + mid):hpf * (j + mid + 1), :]
        xv = x_attn[:, :, j:j + num_frames]
        yv = y_attn[:, :, j + mid]
        yield j, xa, xv, ya, yv


class TrainStep:
    """One optimizer step of the fusion network, autograd-free (see module docstring)."""

    def __init__(self, model, lr=1e-5, loss_coeff=0.001, num_seq=1, betas=(0.9, 0.999), eps=1e-8,
                 process_group=None, sync_bn=False, grad_wire_dtype=None, max_grad_norm=None, audio_loss=None, weight_decay=0.0,
                 decay_filter=None, ema_decay=None, ema_warmup=False, skip_nonfinite=False, wave_loss=None, wave_weight=1.0):
        """`audio_loss`: None trains on the reference's MSE of the STFT planes (ops.mse_pair); a maavss_amd.SpectralLoss replaces that
        term by the power-law compressed spectral loss (ops.spectral_loss_pair): `losses` keeps its three positions (losses[0] is the
        new audio loss, losses[1] the attention MSE by mse_pair's own kernel) and `loss_parts` holds the magnitude and the complex
        mean (device f64 [2]) that losses[0] mixes.
        `max_grad_norm`: FusedAdam's gradient-norm clipping.  It runs once per optimizer step, in the `last` window after the
        all-reduce has finished, on the accumulated, summed gradient times 1 / world -- the norm of the AVERAGED gradient, as DDP
        followed by clip_grad_norm_ gives; every rank computes it from identical bytes, so there is no extra collective.
        `lr` (a float or a maavss_amd.LRSchedule), `weight_decay`, `decay_filter`, `ema_decay`, `ema_warmup`, `skip_nonfinite`: FusedAdam's
        (not in the reference; all off by default).  The skip is decided from the same all-reduced gradient bytes on every rank, so the
        ranks agree without a collective.
        `wave_loss`: None, or a maavss_amd.WaveformLoss whose STFT has the model's n_bins.  sliding_window_step then adds
        wave_weight times the mean over the batch of the clip's SI-SDR / SNR loss -- of the inverse STFT of the num_seq windows' joined
        outputs against the joined targets -- to its objective; `wave` holds the evaluation (device f64: "rows" [B, 5], "loss").
        wave_weight = 0 evaluates and reports the loss without adding its gradient.  The windows' backward passes then run after all
        forwards, so num_seq sets of saved activations are alive at once (README.md has the measured peak)."""
        if wave_loss is not None:
            if not isinstance(wave_loss, WaveformLoss):
                raise ValueError(f"wave_loss must be None or a maavss_amd.WaveformLoss, got {wave_loss!r}")
            if wave_loss.stft.n_bins() != model.n_bins:
                raise ValueError(f"wave_loss: its STFT has n_bins() = {wave_loss.stft.n_bins()}, the model has n_bins = {model.n_bins}")
        if isinstance(wave_weight, bool) or not isinstance(wave_weight, (int, float)) or not math.isfinite(wave_weight) or wave_weight < 0:
            raise ValueError(f"wave_weight must be a finite number >= 0, got {wave_weight!r}")
        self.wave_loss, self.wave_weight = wave_loss, float(wave_weight)
        self.wave = None
        self.model = model
        self.flat = FlatParams(model)
        self.opt = FusedAdam(self.flat, lr, betas, eps, max_grad_norm=max_grad_norm, weight_decay=weight_decay, decay_filter=decay_filter,
                             ema_decay=ema_decay, ema_warmup=ema_warmup, skip_nonfinite=skip_nonfinite)
        self.loss_coeff, self.num_seq = loss_coeff, num_seq
        self.sync = GradSync(self.flat.grads, self.flat.fusion_end, process_group, flat=self.flat, wire_dtype=grad_wire_dtype)
        # replicas start identical: rank 0's weights (one flat buffer) and BatchNorm buffers, like DDP's constructor
        self.sync.broadcast([self.flat.params] + [b for _, b in model.named_buffers()])
        if self.opt.ema is not None and self.sync.enabled:
            self.opt.ema_reset()                      # the average starts from the broadcast weights
        if sync_bn and self.sync.enabled:
            model.set_bn_sync(self.sync.sum_)
        if audio_loss is not None and not isinstance(audio_loss, SpectralLoss):
            raise ValueError(f"audio_loss must be None or a maavss_amd.SpectralLoss, got {audio_loss!r}")
        self.audio_loss = audio_loss
        self.losses = None
        self.loss_parts = None

    def __call__(self, x_a, x_v, y_a, y_v, optimizer_step=True, accumulate=False, last=True):
        """One window: forward, loss / num_seq, backward.  `accumulate` adds into the flat gradient buffer instead of
        overwriting it; the gradient all-reduce and Adam run only when `last` (sliding_window_step drives both).
        requires_grad is read at every call (toggle_* between steps take effect, as with autograd)."""
        if self.wave_loss is not None:
            raise ValueError("with wave_loss set the step is sliding_window_step (the loss needs the whole clip; a single window is a clip "
                             "of num_seq = 1 there)")
        m = self.model
        need = {n: bool(p.requires_grad) for n, p in m.named_parameters()}
        if not accumulate:
            # gradients this step does not produce must not carry over (the engine overwrites the ones it does produce)
            self.flat.touched.clear()
        (a, v, fused), sv = m._engine_forward(x_a, x_v, train=True)
        self.outputs = (a, v, fused)
        if self.audio_loss is None:
            self.losses, d_a, d_v = ops.mse_pair(a, y_a.contiguous(), v, y_v.contiguous(), self.loss_coeff, self.num_seq)
        else:
            self.losses, d_a, d_v, self.loss_parts = ops.spectral_loss_pair(a, y_a.contiguous(), v, y_v.contiguous(), self.loss_coeff,
                                                                            self.audio_loss, self.num_seq)
        if last:
            self.sync.begin(n for n in m._param_names if need.get(n, False))
        out = m._engine_backward(sv, d_a, d_v, None, need, grads=self.flat.grad_views, accumulate=accumulate,
                                 on_fusion_done=self.sync.start_fusion if last else None,
                                 on_grad=self.sync.grad_ready if last else None)
        self.flat.mark(out.keys())
        if last:
            self.sync.finish()
            if optimizer_step:
                self.opt.step(grad_scale=1.0 / self.sync.world)
        return self.losses

    def ema_weights(self):
        """FusedAdam.ema_weights(): inside the block the model runs the averaged weights (and the live BatchNorm statistics)."""
        return self.opt.ema_weights()

    def sliding_window_step(self, x_stft, y_stft, x_attn, y_attn, num_frames, hops_per_frame, collect=False):
        """The reference's optimizer step over `num_seq` overlapping windows (train_avse_frames.py:143-181):
        window j takes frames [j, j + num_frames) of x_attn [B,1,T,H,W] and the matching STFT frames of x_stft
        [B,2,T_a,F]; its targets are attention frame j + idx_mid of y_attn and STFT frames of the same video frame
        of y_stft, idx_mid = (num_seq - 1) // 2 (:105).  Every window contributes loss / num_seq to the gradients
        (accumulated in the flat buffer); ONE gradient all-reduce and ONE Adam step follow.  Returns the last
        window's (a_loss, v_loss, loss) like the reference logs (:183-188) and, with `collect`, the stitched
        outputs (output_stft [B,2,hpf*num_seq,F], output_attn [B,1,num_seq,H,W]) of its callback (:150-176)."""
        if self.wave_loss is not None:
            return self._clip_step(x_stft, y_stft, x_attn, y_attn, num_frames, hops_per_frame, collect)
        ns = self.num_seq
        outs_a, outs_v = [], []
        for j, xa, xv, ya, yv in sliding_windows(x_stft, y_stft, x_attn, y_attn, num_frames, hops_per_frame, ns):
            self(xa, xv, ya, yv, accumulate=j > 0, last=j == ns - 1)
            if collect:
                outs_a.append(self.outputs[0])
                outs_v.append(self.outputs[1])
        if collect:
            return self.losses, torch.cat(outs_a, dim=2), torch.stack(outs_v, dim=2)
        return self.losses

    def _clip_step(self, x_stft, y_stft, x_attn, y_attn, num_frames, hops_per_frame, collect):
        """sliding_window_step with `wave_loss`: the objective is (1 / num_seq) sum_j (a_loss_j + loss_coeff v_loss_j), what the step
        optimises without it, plus wave_weight times the mean over the batch of the clip's waveform loss.  All forwards first (every
        window keeps its saved state; BatchNorm's running statistics move once per window, as ever), then the loss of the joined
        outputs [B,2,hpf*num_seq,F] against the joined targets, whose gradient the kernel adds to the windows' d_a, then the backwards
        in window order; the gradient all-reduce and Adam run in the last one.  `losses` stays the last window's three numbers,
        without the wave term."""
        m, ns, hpf = self.model, self.num_seq, hops_per_frame
        need = {n: bool(p.requires_grad) for n, p in m.named_parameters()}
        self.flat.touched.clear()
        saved, outs_a, outs_v, d_vs, d_all = [], [], [], [], None
        for j, xa, xv, ya, yv in sliding_windows(x_stft, y_stft, x_attn, y_attn, num_frames, hpf, ns):
            (a, v, fused), sv = m._engine_forward(xa, xv, train=True)
            self.outputs = (a, v, fused)
            if d_all is None:
                d_all = torch.empty((ns,) + tuple(a.shape), device=a.device, dtype=torch.float32)      # the windows' d_a, one block each
            if self.audio_loss is None:
                self.losses, _, d_v = ops.mse_pair(a, ya.contiguous(), v, yv.contiguous(), self.loss_coeff, ns, d_a=d_all[j])
            else:
                self.losses, _, d_v, self.loss_parts = ops.spectral_loss_pair(a, ya.contiguous(), v, yv.contiguous(), self.loss_coeff,
                                                                              self.audio_loss, ns, d_a=d_all[j])
            saved.append(sv)
            outs_a.append(a)
            outs_v.append(v)
            d_vs.append(d_v)
        mid = (ns - 1) // 2
        pred = torch.cat(outs_a, dim=2)
        tgt = y_stft[:, :, hpf * mid:hpf * (mid + ns), :]
        if self.wave_weight > 0.0:
            res = self.wave_loss(pred, tgt, grad_scale=self.wave_weight / pred.shape[0], into=d_all)
        else:
            res = self.wave_loss(pred, tgt)
        self.wave = {"rows": res["rows"], "loss": res["loss"]}
        for j in range(ns):
            last = j == ns - 1
            if last:
                self.sync.begin(n for n in m._param_names if need.get(n, False))
            out = m._engine_backward(saved[j], d_all[j], d_vs[j], None, need, grads=self.flat.grad_views, accumulate=j > 0,
                                     on_fusion_done=self.sync.start_fusion if last else None,
                                     on_grad=self.sync.grad_ready if last else None)
            saved[j] = None
            self.flat.mark(out.keys())
        self.sync.finish()
        self.opt.step(grad_scale=1.0 / self.sync.world)
        if collect:
            return self.losses, pred, torch.stack(outs_v, dim=2)
        return self.losses
