"""TEST INFRASTRUCTURE ONLY -- float64 restatement of maavss_amd.Mixer's definition (maavss_amd/mixer.py, include/maavss.h).

    s_b[n]  = sum_k pool[partners[b, k]][n]                       over the slots that are not -1
    Pc_b    = mean_n audio_b[n]^2,  Pi_b = mean_n s_b[n]^2
    g_b     = 10^(-snr_db_b / 20) sqrt(Pc_b / Pi_b);  0 when the clip has no partner, Pi_b == 0 or Pc_b == 0
    y       = STFT(audio)    (oracle.stft_ref_cpu.stft_direct_f64: L // hop frames), times 1 / (max|y_b| + 1e-7) when normalised
    x       = y + (g_b c_b) STFT(s_b) + sigma noise,   c_b = 1 or that same 1 / (max|y_b| + 1e-7)
    mixture = audio + g_b s_b

Also the inputs the CPU and GPU test files share (CASES, partner tables): the CPU file checks on them that the float32 chain stays
inside the gate the GPU file holds the kernels to.
"""
import math

import torch

from oracle import stft_ref_cpu as sref

U = 2.0 ** -24


def gather_sum(pool, partners):
    """-> s [B, L] float64."""
    pool = pool.double()
    s = torch.zeros(partners.shape[0], pool.shape[1], dtype=torch.float64)
    for b in range(partners.shape[0]):
        for k in range(partners.shape[1]):
            p = int(partners[b, k])
            if p >= 0:
                s[b] += pool[p]
    return s


def abs_sum(pool, partners):
    """-> A [B, L] float64 = sum_k |pool[partners[b, k]]|: what the rounding of the float32 gather-sum is relative to."""
    return gather_sum(pool.abs(), partners)


def powers(audio, pool, partners):
    return audio.double().pow(2).mean(1), gather_sum(pool, partners).pow(2).mean(1)


def gain(audio, pool, partners, snr_db):
    pc, pi = powers(audio, pool, partners)
    factor = torch.pow(10.0, -torch.as_tensor(snr_db, dtype=torch.float64) / 20.0)
    live = (partners >= 0).any(1) & (pc > 0) & (pi > 0)
    return torch.where(live, factor * torch.sqrt(pc / torch.where(live, pi, torch.ones_like(pi))), torch.zeros_like(pc))


def gain_bound(audio, pool, partners, threads=256):
    """Relative error bound of the float32 gain, per clip [B] (derivation: tests/test_mixer_gpu.py)."""
    n_seq = -(-audio.shape[1] // threads)
    s, a = gather_sum(pool, partners), abs_sum(pool, partners)
    k_live = (partners >= 0).sum(1).double()
    pi = s.pow(2).sum(1)
    form = (k_live - 1).clamp_min(0) * (s.abs() * a).sum(1) / torch.where(pi > 0, pi, torch.ones_like(pi))
    return (n_seq + math.log2(threads) + 1 + 4 + form) * U


def mixture(audio, pool, partners, g):
    return audio.double() + g.double()[:, None] * gather_sum(pool, partners)


def realised_snr_db(audio, mix):
    """10 log10(Pc / P(mixture - clean)) in float64."""
    a = audio.double()
    return 10.0 * torch.log10(a.pow(2).mean(1) / (mix.double() - a).pow(2).mean(1))


def example(audio, pool, partners, g, fft_len, hop, sigma, noise, normalized=True, trim=False, normalize_output=False):
    """-> (x, y, term) float64 [B, 2, L // hop, F]; term = g_b c_b STFT(s_b), the part of x the gain's error scales."""
    f = fft_len // 2 + (0 if trim else 1)
    y = sref.stft_direct_f64(audio, fft_len, hop, normalized, n_bins=f)
    inter = sref.stft_direct_f64(gather_sum(pool, partners), fft_len, hop, normalized, n_bins=f)
    c = torch.ones(audio.shape[0], dtype=torch.float64)
    if normalize_output:
        c = 1.0 / (y.abs().flatten(1).max(1).values + 1e-7)
        y = y * c[:, None, None, None]
    term = (g.double() * c)[:, None, None, None] * inter
    x = y + term
    if noise is not None:
        x = x + sigma * noise.double()
    return x, y, term


# ---- shared inputs --------------------------------------------------------------------------------------------------------------
HOP, LENGTH, BATCH, POOL = 66, 594, 5, 3          # 9 frames: an odd count leaves a half-empty pair, 45 frames an odd total
SNRS = [-5.0, 0.0, 10.0, 30.0, 0.0]
SIGMA = 0.1
# partners[pool is the batch?][K]: -1 holes in every table, a clip without any partner in most
PARTNERS = {
    (True, 1): [[1], [2], [3], [4], [-1]],
    (True, 2): [[1, 2], [-1, 0], [4, -1], [0, 1], [2, 3]],
    (True, 4): [[1, 2, 3, 4], [0, -1, 2, -1], [-1, -1, -1, -1], [4, 0, 1, 2], [3, -1, -1, 0]],
    (False, 1): [[0], [1], [2], [-1], [0]],
    (False, 2): [[0, 1], [2, -1], [-1, 1], [2, 0], [1, 2]],
    (False, 4): [[0, 1, 2, -1], [-1, 2, -1, 0], [1, -1, -1, -1], [-1, -1, -1, -1], [2, 0, -1, 1]],
}
# (fft_len, trim_stft_end, normalize_output_fft, K, pool is the batch): every fft_len with both trims and both normalisations, K and the
# pool cycling through them
CASES = [(fft, trim, norm, (1, 2, 4)[(i + j + 2 * k) % 3], bool((i + j + k) % 2))
         for i, fft in enumerate((256, 512, 1024)) for j, trim in enumerate((False, True)) for k, norm in enumerate((False, True))]


def inputs(k, own_pool, batch=BATCH, length=LENGTH):
    """-> (audio [B, L], pool or None, partners int32 [B, K], snr_db f32 [B]) on the CPU."""
    audio = sref.synthetic_audio(batch, length, 11)
    pool = None if own_pool else sref.synthetic_audio(POOL, length, 12)
    partners = torch.tensor(PARTNERS[(own_pool, k)], dtype=torch.int32)
    return audio, pool, partners, torch.tensor(SNRS, dtype=torch.float32)


def noise_for(batch, length, hop, f, seed=13):
    return torch.randn(batch, 2, length // hop, f, generator=torch.Generator().manual_seed(seed))


def gate(normalize_output):
    """tests/test_stft_gpu.py's gate, relative to the largest coefficient: 5e-6 at |y| <= 0.5 -> 1e-5; 2e-5 with normalize_output_fft
    (there max|y| = 1)."""
    return 2e-5 if normalize_output else 1e-5
