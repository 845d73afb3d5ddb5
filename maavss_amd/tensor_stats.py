"""Per-tensor statistics of the flat buffers, on the device: what gradient-norm clipping and `wandb.watch` need on the
autograd-free path.

The reference's trainers call `wandb.watch(model, mse_loss, log="all", log_freq=300)` (train_avse_frames.py:108), which hangs
autograd hooks on every parameter; under `TrainStep` no hook ever fires.  Here one segmented reduction over `FlatParams.grads` /
`FlatParams.params` (csrc/tensor_stats.hip) gives, per tensor: sum of squares (f64), min, max, NaN / +inf / -inf counts and a
`torch.histc`-equal histogram; and over a chosen subset the global gradient norm and `clip_grad_norm_`'s coefficient, left on the
device for `maavss_adam_step_dscale`.

* `plan_chunks`  -- the host-side chunk planner (pure, no device)
* `TensorStats`  -- chunk table, mask, outputs and workspace of one FlatParams layout; `.run()` enqueues, `.to_host()` copies once
* `ModelWatch`   -- the stand-in for `wandb.watch`: every `log_freq` steps a dict of `(counts, edges)` histograms
"""
import numpy as np

from ._lib import MaavssError, call, ptr, query, require_cuda, stream_ptr, workspace

MAX_BINS = 1024


def chunk_len():
    """CH: the longest chunk one workgroup of pass 1 reduces (a constant of the library)."""
    return int(query("maavss_tensor_stats_chunk"))


def plan_chunks(offsets, numels, ch):
    """[(segment, start, length)] in buffer order: segment s = [offsets[s], offsets[s] + numels[s]) cut into pieces of at most `ch`
    elements; no piece crosses a segment boundary, every element is in exactly one piece.  Segments must not overlap and must be
    given in buffer order (FlatParams.names order)."""
    if ch < 1:
        raise ValueError("ch must be >= 1")
    rows, end = [], 0
    for s, (o, k) in enumerate(zip(offsets, numels)):
        o, k = int(o), int(k)
        if o < end or k < 0:
            raise ValueError(f"segment {s} [{o}, +{k}) overlaps its predecessor or is out of buffer order")
        end = o + k
        for a in range(o, end, ch):
            rows.append((s, a, min(ch, end - a)))
    return rows


def _numel(shape):
    k = 1
    for d in shape:
        k *= d
    return k


def _align(n, a):
    return (n + a - 1) // a * a


class TensorStats:
    """Statistics of one flat f32 buffer of a `FlatParams` layout (`flat.grads` or `flat.params`), one segment per parameter tensor.

    Everything `.run()` needs lives on the device and is built once: the chunk table, the selection mask, the workspace and ONE output
    buffer, so `.to_host()` is a single device-to-host copy.  `.run()` only enqueues launches on the current stream."""

    def __init__(self, flat, bins=64):
        import torch
        if not 1 <= int(bins) <= MAX_BINS:
            raise ValueError(f"bins must be in 1..{MAX_BINS}")
        self.flat, self.bins = flat, int(bins)
        self.names = list(flat.names)
        self.index = {n: i for i, n in enumerate(self.names)}
        s = len(self.names)
        self._off = np.array([flat.offsets[n] for n in self.names], dtype=np.int64)
        self._num = np.array([_numel(flat.shapes[n]) for n in self.names], dtype=np.int64)
        self.ch = chunk_len()
        rows = plan_chunks(self._off, self._num, self.ch)
        first = np.zeros(s + 1, dtype=np.int32)
        for sg, _, _ in rows:
            first[sg + 1] += 1
        first = np.cumsum(first, dtype=np.int64).astype(np.int32)
        dev = flat.params.device
        self.n_chunks = len(rows)
        self._chunks = torch.tensor(rows if rows else [(0, 0, 0)], dtype=torch.int64).reshape(-1, 3).to(dev)
        self._first = torch.from_numpy(first).to(dev)
        self._mask = torch.ones(s, dtype=torch.int32, device=dev)
        self._mask_key = None                      # names the mask on the device stands for (None = all)
        self._ws_bytes = int(query("maavss_tensor_stats_ws_bytes", self.n_chunks, s, self.bins))
        self._ws = workspace(self._ws_bytes, dev)      # the entry point asks for ws_bytes and no more: no spare element
        # one output buffer: [sumsq f64 x S | total_sumsq f64 | min f32 x S | max f32 x S | norm f32 | scale f32 | nonfinite i32 x 3S | hist i32 x S*bins]
        self._lay, o = {}, 0
        for key, dt, cnt in (("sumsq", np.float64, s), ("total_sumsq", np.float64, 1), ("min", np.float32, s), ("max", np.float32, s),
                             ("norm", np.float32, 1), ("scale", np.float32, 1), ("nonfinite", np.int32, 3 * s),
                             ("hist", np.int32, s * self.bins)):
            self._lay[key] = (o, np.dtype(dt), cnt)
            o = _align(o + cnt * np.dtype(dt).itemsize, 8)
        self._out = torch.zeros(o, dtype=torch.uint8, device=dev)
        tdt = {np.dtype(np.float64): torch.float64, np.dtype(np.float32): torch.float32, np.dtype(np.int32): torch.int32}
        self._views = {k: self._out[a:a + c * d.itemsize].view(tdt[d]) for k, (a, d, c) in self._lay.items()}
        self._views["nonfinite"] = self._views["nonfinite"].view(s, 3)
        self._views["hist"] = self._views["hist"].view(s, self.bins)
        self._had_hist = False

    def _set_mask(self, names):
        import torch
        key = None if names is None else tuple(sorted(self.index[n] for n in set(names)))
        if key == self._mask_key:
            return
        m = np.ones(len(self.names), dtype=np.int32) if key is None else np.zeros(len(self.names), dtype=np.int32)
        if key is not None:
            m[list(key)] = 1
        self._mask.copy_(torch.from_numpy(m))      # only when the selection changes (a freeze / unfreeze), never per step
        self._mask_key = key

    def run(self, buffer, names=None, hist=True, max_norm=None, grad_scale=1.0):
        """Enqueue the statistics of `buffer` (`flat.grads` or `flat.params`) on the current stream; nothing is read back.
        `names` selects the tensors whose sum of squares makes `norm` (None = all); it changes nothing else.  `max_norm` (None = no
        clip) and `grad_scale` give `norm` = |grad_scale * g| and `scale` = grad_scale * min(1, max_norm / (norm + 1e-6)).
        Returns the device tensors sumsq [S] f64, min / max [S], nonfinite [S,3] (NaN, +inf, -inf), hist [S, bins] (None without
        `hist`), norm, scale [1] (None without `max_norm`).  They are views of one buffer the next run() overwrites."""
        require_cuda(buffer)
        if buffer.dtype != self.flat.params.dtype or buffer.numel() != self.flat.total or not buffer.is_contiguous():
            raise MaavssError("TensorStats.run: buffer must be the flat f32 buffer of the layout (flat.grads or flat.params)")
        if max_norm is not None and not float(max_norm) >= 0.0:
            raise ValueError("max_norm must be >= 0")
        self._set_mask(names)
        v = self._views
        clip = max_norm is not None
        call("maavss_tensor_stats", ptr(buffer), buffer.numel(), ptr(self._chunks), self.n_chunks, ptr(self._first),
             self._off.ctypes.data, self._num.ctypes.data, len(self.names), ptr(self._mask), ptr(v["sumsq"]), ptr(v["min"]), ptr(v["max"]),
             ptr(v["nonfinite"]), ptr(v["hist"]) if hist else None, self.bins, float(max_norm) if clip else -1.0, float(grad_scale),
             ptr(v["total_sumsq"]), ptr(v["norm"]), ptr(v["scale"]), ptr(self._ws), self._ws_bytes, stream_ptr())
        self._had_hist = bool(hist)
        return {"sumsq": v["sumsq"], "min": v["min"], "max": v["max"], "nonfinite": v["nonfinite"], "hist": v["hist"] if hist else None,
                "norm": v["norm"] if clip else None, "scale": v["scale"] if clip else None}

    @property
    def norm(self):
        return self._views["norm"]

    @property
    def scale(self):
        return self._views["scale"]

    def _unpack(self, raw):
        """raw: the output buffer as a host uint8 numpy array -> {name: {...}}"""
        f = {k: raw[a:a + c * d.itemsize].view(d) for k, (a, d, c) in self._lay.items()}
        nonf = f["nonfinite"].reshape(-1, 3)
        hist = f["hist"].reshape(-1, self.bins)
        out = {}
        for i, n in enumerate(self.names):
            lo, hi = float(f["min"][i]), float(f["max"][i])
            if lo == hi:
                lo, hi = lo - 1.0, hi + 1.0
            out[n] = {"norm": float(np.sqrt(f["sumsq"][i])), "min": float(f["min"][i]), "max": float(f["max"][i]),
                      "nan": int(nonf[i, 0]), "posinf": int(nonf[i, 1]), "neginf": int(nonf[i, 2]),
                      "counts": hist[i].copy() if self._had_hist else None,
                      "edges": np.linspace(lo, hi, self.bins + 1) if self._had_hist else None}
        return out

    def to_host(self):
        """{name: {norm, min, max, nan, posinf, neginf, counts, edges}} of the last run(), after ONE device-to-host copy (which waits
        for the stream).  `norm` is the tensor's own 2-norm (unscaled); `counts` int32 [bins] and `edges` f64 [bins + 1] are what
        numpy.histogram returns (None when the run had no histogram); a tensor without a finite element has NaN min / max / edges."""
        return self._unpack(self._out.cpu().numpy())


def to_host_all(stats):
    """[s.to_host() for s in stats] with one device-to-host copy for all of them when they are TensorStats."""
    import torch
    stats = list(stats)
    if not stats or not all(isinstance(s, TensorStats) for s in stats):
        return [s.to_host() for s in stats]
    raw = torch.cat([s._out for s in stats]).cpu().numpy()
    out, o = [], 0
    for s in stats:
        k = s._out.numel()
        out.append(s._unpack(raw[o:o + k]))
        o += k
    return out


class ModelWatch:
    """Stand-in for `wandb.watch(model, criterion, log="all", log_freq=300)` on the autograd-free path.

        watch = maavss_amd.ModelWatch(step, log_freq=300)          # a TrainStep, a FusedAdam or a FlatParams
        ...
        losses = step(x_a, x_v, y_a, y_v)
        logs = watch.after_step()
        if logs is not None:
            wandb.log({k: wandb.Histogram(np_histogram=v) for k, v in logs.items() if not k.startswith("nonfinite/")})

    `after_step()` returns None, or every `log_freq` calls a dict with `gradients/<name>` and `parameters/<name>` -> `(counts, edges)`
    numpy arrays (`log`: "gradients", "parameters" or "all"), and `nonfinite/<kind>/<name>` -> {"nan", "posinf", "neginf"} for a
    tensor that holds any.  A tensor without a finite element has no histogram entry.  The statistics are reduced on the device
    (two passes over each flat buffer); one device-to-host copy brings them over, never the tensors.  wandb is not imported."""

    def __init__(self, step_or_optimizer, log_freq=300, bins=64, log="all", stats_cls=TensorStats):
        if log not in ("gradients", "parameters", "all"):
            raise ValueError('log must be "gradients", "parameters" or "all"')
        if int(log_freq) < 1:
            raise ValueError("log_freq must be >= 1")
        self.flat = getattr(step_or_optimizer, "flat", step_or_optimizer)
        self.log_freq, self.bins = int(log_freq), int(bins)
        self.kinds = ("gradients", "parameters") if log == "all" else (log,)
        self.stats = {k: stats_cls(self.flat, bins=self.bins) for k in self.kinds}
        self.calls = 0

    def _buffer(self, kind):
        return self.flat.grads if kind == "gradients" else self.flat.params

    def after_step(self):
        self.calls += 1
        if self.calls % self.log_freq:
            return None
        for k in self.kinds:
            self.stats[k].run(self._buffer(k), hist=True)
        logs = {}
        for k, host in zip(self.kinds, to_host_all(self.stats[k] for k in self.kinds)):
            for n, d in host.items():
                if d["nan"] or d["posinf"] or d["neginf"]:
                    logs[f"nonfinite/{k}/{n}"] = {"nan": d["nan"], "posinf": d["posinf"], "neginf": d["neginf"]}
                if d["counts"] is not None and d["min"] == d["min"]:
                    logs[f"{k}/{n}"] = (d["counts"], d["edges"])
        return logs
