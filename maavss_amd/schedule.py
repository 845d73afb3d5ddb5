"""Learning-rate schedule of FusedAdam / TrainStep (not in the reference, which trains at one fixed rate: train_avse_frames.py:92).

The rate is an argument of the optimizer kernel, so a schedule is host arithmetic only: float64, no device work, no synchronisation.
`FusedAdam(lr=LRSchedule(...))` asks it for the rate of every optimizer step; the object owns its state and goes into a checkpoint
through `state_dict()` (checkpoint.save_checkpoint(schedule_dict=...)).
"""
import math

KINDS = ("constant", "linear", "cosine")


class LRSchedule:
    """lr(t) of optimizer step t (counted from 0):

        t <  warmup_steps          base_lr * (t + 1) / (warmup_steps + 1)       linear warm-up from base_lr / (warmup_steps + 1)
        t >= warmup_steps          "constant": base_lr
                                   "linear":   base_lr + (min_lr - base_lr) * x          x = (t - warmup_steps) / (total_steps - warmup_steps)
                                   "cosine":   min_lr + (base_lr - min_lr) * (1 + cos(pi x)) / 2
        t >= total_steps           min_lr for "linear" and "cosine" (the rate stays constant from there on)

    all times `scale`, a plain attribute (1.0) that a plateau rule in user code may lower.  `t` is the number of rates handed out by
    next_lr() so far; both are part of the state."""

    def __init__(self, base_lr, warmup_steps=0, total_steps=None, kind="constant", min_lr=0.0):
        if kind not in KINDS:
            raise ValueError(f"kind must be one of {KINDS}")
        if not float(base_lr) >= 0.0 or not float(min_lr) >= 0.0:
            raise ValueError("base_lr and min_lr must be >= 0")
        if int(warmup_steps) < 0:
            raise ValueError("warmup_steps must be >= 0")
        if kind != "constant":
            if total_steps is None:
                raise ValueError(f'kind "{kind}" needs total_steps')
            if int(total_steps) <= int(warmup_steps):
                raise ValueError("total_steps must be larger than warmup_steps")
        self.base_lr, self.min_lr = float(base_lr), float(min_lr)
        self.warmup_steps = int(warmup_steps)
        self.total_steps = None if total_steps is None else int(total_steps)
        self.kind = kind
        self.scale = 1.0
        self.t = 0          # the optimizer step whose rate next_lr() hands out next

    def lr(self, t):
        t = int(t)
        if t < 0:
            raise ValueError("t counts optimizer steps from 0")
        w = self.warmup_steps
        if t < w:
            r = self.base_lr * (t + 1) / (w + 1)
        elif self.kind == "constant":
            r = self.base_lr
        elif t >= self.total_steps:
            r = self.min_lr
        else:
            x = (t - w) / (self.total_steps - w)
            if self.kind == "linear":
                r = self.base_lr + (self.min_lr - self.base_lr) * x
            else:
                r = self.min_lr + (self.base_lr - self.min_lr) * 0.5 * (1.0 + math.cos(math.pi * x))
        return r * float(self.scale)

    __call__ = lr

    def next_lr(self):
        """The rate of optimizer step `t`, then t += 1: what FusedAdam.step() calls once per step (a skipped step included)."""
        r = self.lr(self.t)
        self.t += 1
        return r

    def state_dict(self):
        return {"base_lr": self.base_lr, "warmup_steps": self.warmup_steps, "total_steps": self.total_steps, "kind": self.kind,
                "min_lr": self.min_lr, "scale": float(self.scale), "t": int(self.t)}

    def load_state_dict(self, sd):
        fresh = LRSchedule(sd["base_lr"], sd["warmup_steps"], sd["total_steps"], sd["kind"], sd["min_lr"])      # validates
        self.__dict__.update(fresh.__dict__)
        self.scale = float(sd.get("scale", 1.0))
        self.t = int(sd.get("t", 0))

    def __repr__(self):
        return (f"LRSchedule(base_lr={self.base_lr}, warmup_steps={self.warmup_steps}, total_steps={self.total_steps}, kind={self.kind!r}, "
                f"min_lr={self.min_lr}, scale={self.scale})")
