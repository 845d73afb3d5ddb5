"""TEST INFRASTRUCTURE ONLY -- float64 twins and derived error bounds for the small f32 kernels (LSTM saved state,
adaptive average pool, channel sum).  Plain torch on the CPU; tests/test_f32_edges_cpu.py checks each of them against
torch's own operators before the GPU tests rely on them."""
import torch

U = 2.0 ** -24          # unit roundoff of float32


# ---------------------------------------------------------------------------------------------- LSTM
def lstm_bidir_steps_f64(gx, whh_f, whh_b):
    """Step-by-step twin of a bias-free bidirectional LSTM layer with zero initial state (gate order i, f, g, o).
    gx [B, L, 2, 4, H] = the input projections; whh_* [4H, H].  Returns float64
    av [B, L, 2H], hp [B, L, 2, H] (hidden state that ENTERED step t), gs [B, L, 2, 4, H] (gates after their
    nonlinearity), cs [B, L, 2, H] (cell state after step t)."""
    gx = gx.double()
    b, l, _, _, h = gx.shape
    av, hp = gx.new_zeros(b, l, 2 * h), gx.new_zeros(b, l, 2, h)
    gs, cs = gx.new_zeros(b, l, 2, 4, h), gx.new_zeros(b, l, 2, h)
    for d, whh in enumerate((whh_f.double(), whh_b.double())):
        hprev, cprev = gx.new_zeros(b, h), gx.new_zeros(b, h)
        for t in (range(l) if d == 0 else range(l - 1, -1, -1)):
            pre = gx[:, t, d] + (hprev @ whh.T).view(b, 4, h)
            i, f, g, o = pre[:, 0].sigmoid(), pre[:, 1].sigmoid(), pre[:, 2].tanh(), pre[:, 3].sigmoid()
            c = f * cprev + i * g
            hp[:, t, d], cs[:, t, d] = hprev, c
            gs[:, t, d] = torch.stack([i, f, g, o], 1)
            hprev, cprev = o * c.tanh(), c
            av[:, t, d * h:(d + 1) * h] = hprev
    return av, hp, gs, cs


# ---------------------------------------------------------------------------------------------- adaptive average pool
def pool_windows(n_in, n_out):
    """[(start, end)] of torch's AdaptiveAvgPool windows along one axis: floor(o n_in / n_out) .. ceil((o + 1) n_in / n_out)."""
    return [((o * n_in) // n_out, ((o + 1) * n_in + n_out - 1) // n_out) for o in range(n_out)]


def adaptive_pool_fwd_bound(x, ho, wo):
    """x [B, C, H, W] -> bound [B, C, ho, wo] on |f32 result - exact| = (n + 1) u mean|x over the window|, n = the
    window's element count: n - 1 additions in any order and one division, each one rounding of a partial result that
    |x|'s sum bounds."""
    ax = x.double().abs()
    out = ax.new_zeros(*x.shape[:2], ho, wo)
    for oy, (y0, y1) in enumerate(pool_windows(x.shape[2], ho)):
        for ox, (x0, x1) in enumerate(pool_windows(x.shape[3], wo)):
            n = (y1 - y0) * (x1 - x0)
            out[:, :, oy, ox] = (n + 1) * U * ax[:, :, y0:y1, x0:x1].sum((2, 3)) / n
    return out


def adaptive_pool_bwd_bound(dout, h, w):
    """dout [B, C, ho, wo] -> bound [B, C, h, w] on the input gradient: (n + 1) u sum|dout / count| over the windows that
    cover the pixel, n = their number plus one (one division per window, then their sum)."""
    ad = dout.double().abs()
    acc, cover = ad.new_zeros(*dout.shape[:2], h, w), torch.zeros(h, w, dtype=torch.float64)
    for oy, (y0, y1) in enumerate(pool_windows(h, dout.shape[2])):
        for ox, (x0, x1) in enumerate(pool_windows(w, dout.shape[3])):
            acc[:, :, y0:y1, x0:x1] += ad[:, :, oy, ox][:, :, None, None] / ((y1 - y0) * (x1 - x0))
            cover[y0:y1, x0:x1] += 1
    return (cover + 2) * U * acc


# ---------------------------------------------------------------------------------------------- channel sum
def channel_sum_bound(x, prior=None):
    """x [rows, C] (any layout), prior [C] or None -> (exact float64 result [C], bound [C]).  (rows - 1) u sum|x| holds
    for every summation order of the rows; adding a prior `out` (beta = 1) is one more rounding of the result."""
    x64 = x.double()
    want = x64.sum(0)
    bound = (x.shape[0] - 1) * U * x64.abs().sum(0)
    if prior is not None:
        want = want + prior.double()
        bound = bound + U * want.abs()
    return want, bound
