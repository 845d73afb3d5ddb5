"""Mix-and-separate training examples: the network's input is the clip plus other clips' audio at a chosen signal-to-interferer
ratio, its target the clip's own STFT.  Extends AV_Dataset.add_noise / gen_stft_example (av_dataset.py:217-220, 335-342), whose
only corruption is white noise on the STFT coefficients.  The kernels are maavss_mix_gains, maavss_stft_mix_fwd and maavss_mix_wave
(include/maavss.h, csrc/mix.hip); tests/mix_twin.py restates the definition in float64.

    s_b = sum_k pool[partners[b, k]]                          (-1 = empty slot)
    g_b = 10^(-snr_db_b / 20) sqrt(mean audio_b^2 / mean s_b^2),   0 when the clip has no partner or either power is 0
    y   = STFT(audio), bit for bit what stft(audio, want_x=False) returns
    x   = y + (g_b c_b) STFT(s_b) + noise_std * noise,         c_b = 1, or 1 / (max|y_b| + 1e-7) with normalize_output_fft
    mixture = audio + g_b s_b
"""
import math

import torch

from . import _lib

MAX_INTERFERERS = 4


class Mixer:
    """`mixer = Mixer(stft, interferers=K, snr_db=(lo, hi))`; `x, y = mixer(audio, seed=s)` mixes every clip with K others of the batch.

    The in-kernel noise of `x` is element for element the noise `stft(audio, seed=s)` adds: switching mixing on does not change it."""

    def __init__(self, stft, interferers=1, snr_db=(0.0, 10.0)):
        if isinstance(interferers, bool) or not isinstance(interferers, int) or not 1 <= interferers <= MAX_INTERFERERS:
            raise ValueError(f"interferers must be an integer in [1, {MAX_INTERFERERS}], got {interferers!r}")
        lo, hi = (float(v) for v in snr_db)
        if not (math.isfinite(lo) and math.isfinite(hi)) or lo > hi:
            raise ValueError(f"snr_db must be a finite range (lo, hi) with lo <= hi, got {snr_db!r}")
        self.stft, self.interferers, self.snr_db = stft, interferers, (lo, hi)

    def sample(self, batch, generator, pool_size=None):
        """-> (partners [batch, K] int32, snr_db [batch] f32), CPU tensors drawn from `generator` (a CPU torch.Generator).

        pool_size=None: the pool is the batch and a clip is never its own partner (batch - 1 candidates); otherwise every row of the
        pool is a candidate.  Each clip gets min(K, candidates) distinct partners, uniformly; the remaining slots are -1.
        Draw order: first one torch.rand(batch, float64) for the SNRs (lo + (hi - lo) u), then for clip 0, 1, ... in turn one
        torch.randperm(candidates) whose first K entries are the clip's partners in slot order (with the batch as pool, candidate
        c >= b stands for clip c + 1)."""
        if isinstance(batch, bool) or not isinstance(batch, int) or batch < 1:
            raise ValueError(f"batch must be a positive integer, got {batch!r}")
        if pool_size is not None and (isinstance(pool_size, bool) or not isinstance(pool_size, int) or pool_size < 1):
            raise ValueError(f"pool_size must be a positive integer, got {pool_size!r}")
        lo, hi = self.snr_db
        u = torch.rand(batch, generator=generator, dtype=torch.float64)
        if hi > lo:
            snr = (lo + (hi - lo) * u).to(torch.float32).clamp(_f32_up(lo), _f32_down(hi))      # rounding to f32 must not leave [lo, hi]
        else:
            snr = torch.full((batch,), lo, dtype=torch.float32)
        k = self.interferers
        partners = torch.full((batch, k), -1, dtype=torch.int32)
        cand = batch - 1 if pool_size is None else pool_size
        for b in range(batch):
            pick = torch.randperm(cand, generator=generator)[:k]
            if pool_size is None:
                pick = pick + (pick >= b).to(pick.dtype)
            partners[b, :pick.numel()] = pick.to(torch.int32)
        return partners, snr

    def check(self, audio, partners, snr_db, pool=None, noise=None):
        """Every refusal, from shapes, dtypes and values alone (no device work) -> (partners int32 [B, K], snr_db f64 [B], both on the
        CPU).  `audio` is the [B, L] tensor or, when it does not exist yet, the pair (B, L)."""
        if isinstance(audio, torch.Tensor):
            if audio.dim() != 2 or audio.dtype != torch.float32 or audio.stride(1) != 1 or audio.stride(0) < 0:
                raise ValueError(f"audio must be float32 [B, L] with unit last stride, got {audio.dtype} {tuple(audio.shape)} strides {audio.stride()}")
            b, length = audio.shape
        else:
            b, length = audio
        if b < 1 or length < 1:
            raise ValueError(f"audio needs at least one clip and one sample, got [B, L] = {(b, length)}")
        if pool is None:
            p = b
        else:
            if not isinstance(pool, torch.Tensor) or pool.dim() != 2 or pool.dtype != torch.float32 or pool.stride(1) != 1 or pool.stride(0) < 0:
                raise ValueError(f"pool must be float32 [P, L] with unit last stride, got {getattr(pool, 'dtype', type(pool))} "
                                 f"{tuple(getattr(pool, 'shape', ()))}")
            if pool.shape[1] != length:
                raise ValueError(f"pool clips have {pool.shape[1]} samples, audio clips {length}: the pool must be [P, {length}]")
            if pool.shape[0] < 1:
                raise ValueError("pool is empty")
            if isinstance(audio, torch.Tensor) and pool.device != audio.device:
                raise ValueError(f"pool is on {pool.device}, audio on {audio.device}")
            p = pool.shape[0]
        if not isinstance(partners, torch.Tensor) or partners.dtype != torch.int32 or partners.dim() != 2 or partners.shape[0] != b:
            raise ValueError(f"partners must be an int32 [{b}, K] tensor, got {getattr(partners, 'dtype', type(partners))} "
                             f"{tuple(getattr(partners, 'shape', ()))}")
        if partners.is_cuda:
            raise ValueError("partners must be a CPU tensor (its values are checked on the host, like crop boxes)")
        k = partners.shape[1]
        if not 1 <= k <= MAX_INTERFERERS:
            raise ValueError(f"partners has K = {k} slots per clip, K must be in [1, {MAX_INTERFERERS}]")
        if bool(((partners < -1) | (partners >= p)).any()):
            raise ValueError(f"partners entries must be in [-1, {p}) (-1 = empty slot), got [{int(partners.min())}, {int(partners.max())}]")
        if pool is None and bool((partners == torch.arange(b, dtype=torch.int32)[:, None]).any()):
            raise ValueError("a clip is listed as its own partner (the pool is the batch)")
        if isinstance(snr_db, torch.Tensor) and snr_db.is_cuda:
            raise ValueError("snr_db must be a CPU tensor or a number")
        snr = torch.as_tensor(snr_db, dtype=torch.float64)
        if snr.dim() == 0:
            snr = snr.expand(b)
        if tuple(snr.shape) != (b,):
            raise ValueError(f"snr_db must be a number or a [{b}] tensor, got {tuple(snr.shape)}")
        if not bool(torch.isfinite(snr).all()):
            raise ValueError("snr_db must be finite")
        factor = torch.pow(10.0, -snr / 20.0).to(torch.float32)
        if not bool((torch.isfinite(factor) & (factor > 0)).all()):
            raise ValueError("snr_db is outside the range whose amplitude factor 10^(-snr_db/20) float32 can hold")
        if noise is not None:
            want = (b, 2, length // self.stft.hop, self.stft.n_bins())
            if not isinstance(noise, torch.Tensor) or noise.dtype != torch.float32 or tuple(noise.shape) != want or not noise.is_contiguous():
                raise ValueError(f"noise must be a contiguous float32 {list(want)} tensor, got {getattr(noise, 'dtype', type(noise))} "
                                 f"{tuple(getattr(noise, 'shape', ()))}")
        return partners.contiguous(), snr.contiguous()

    def __call__(self, audio, partners=None, snr_db=None, *, pool=None, noise=None, seed=0, return_mixture=False, return_gain=False):
        """audio [B, L] f32 on the device (rows may be strided, as STFT accepts); partners [B, K] int32 and snr_db [B] (or a number) on
        the CPU, by default self.sample(B, torch.Generator().manual_seed(seed), P); pool [P, L] on the device, by default `audio`.
        -> (x, y[, mixture [B, L]][, gain [B]]).  Everything is checked before any device work; partners and SNRs reach the device
        through pinned memory without a synchronisation, and all work goes to the current stream."""
        if partners is None or snr_db is None:
            drawn = self.sample(audio.shape[0], torch.Generator().manual_seed(seed), None if pool is None else pool.shape[0])
            partners = drawn[0] if partners is None else partners
            snr_db = drawn[1] if snr_db is None else snr_db
        partners, snr = self.check(audio, partners, snr_db, pool, noise)
        _lib.require_cuda(audio, pool, noise)
        st = self.stft
        dev = audio.device
        src = audio if pool is None else pool
        b, length = audio.shape
        k = partners.shape[1]
        n_frames, f = length // st.hop, st.n_bins()
        # the target first: exactly the launches of stft(audio, want_x=False)
        if st.normalize_output_fft:
            _, y, c = st(audio, want_x=False, return_scale=True)
        else:
            (_, y), c = st(audio, want_x=False), None
        # partners and the SNR factors reach the device in one copy through pinned memory, without a synchronisation: on ClipPipeline's
        # side stream a blocking copy would hold the host until the whole extraction queued in front of it had finished
        host = torch.cat([partners.reshape(-1), torch.pow(10.0, -snr / 20.0).to(torch.float32).view(torch.int32)])
        staged = torch.empty(b * (k + 1), device=dev, dtype=torch.int32)
        staged.copy_(host.pin_memory(), non_blocking=True)
        partners_d, factor_d = staged[:b * k], staged[b * k:].view(torch.float32)
        gain = torch.empty(b, device=dev, dtype=torch.float32)
        x = torch.empty_like(y)
        sp = _lib.stream_ptr()
        _lib.call("maavss_mix_gains", _lib.ptr(audio), b, length, audio.stride(0), _lib.ptr(src), src.shape[0], src.stride(0),
                  _lib.ptr(partners_d), k, _lib.ptr(factor_d), _lib.ptr(gain), sp)
        _lib.call("maavss_stft_mix_fwd", _lib.ptr(src), src.shape[0], length, src.stride(0), _lib.ptr(partners_d), k, b,
                  _lib.ptr(st.window), st.fft_len, st.hop, n_frames, f, _lib.ptr(y), _lib.ptr(x), _lib.ptr(noise), float(st.noise_std),
                  int(seed), _lib.ptr(gain), _lib.ptr(c), sp)
        out = [x, y]
        if return_mixture:
            mixture = torch.empty(b, length, device=dev, dtype=torch.float32)
            _lib.call("maavss_mix_wave", _lib.ptr(audio), b, length, audio.stride(0), _lib.ptr(src), src.shape[0], src.stride(0),
                      _lib.ptr(partners_d), k, _lib.ptr(gain), _lib.ptr(mixture), mixture.stride(0), sp)
            out.append(mixture)
        if return_gain:
            out.append(gain)
        return tuple(out)


def _f32_up(v):
    """Smallest float32 >= v."""
    t = torch.tensor(v, dtype=torch.float64).to(torch.float32)
    return float(t) if float(t) >= v else float(torch.nextafter(t, torch.tensor(math.inf, dtype=torch.float32)))


def _f32_down(v):
    """Largest float32 <= v."""
    t = torch.tensor(v, dtype=torch.float64).to(torch.float32)
    return float(t) if float(t) <= v else float(torch.nextafter(t, torch.tensor(-math.inf, dtype=torch.float32)))
