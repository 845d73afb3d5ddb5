"""Engine pieces that AV_Fusion_Model_Frames (avse.py) and AV_Fusion_Model (avfm.py) both use: the channel-padded
BatchNorm2d glue and the BiLSTM block.  Plain functions over maavss_amd.ops; what differs between the two models (tanh
against bias + LeakyReLU, the bias gradients) stays in their own files."""
import torch

from . import ops


def cpad(c):
    """channel count the BatchNorm kernels accept (power of two >= 4; all counts here are powers of two already): a
    2-channel layer runs with two dead channels, which stay exactly zero through BN (gamma = beta = 0), tanh and the backward pass."""
    return max(c, 4)


def pad_c(v, c, fill=0.0):
    """per-channel vector v padded to c entries"""
    if v.shape[0] == c:
        return v
    return torch.cat((v, torch.full((c - v.shape[0],), fill, device=v.device, dtype=v.dtype)))


def bn_stats_padded(y, bn, c_real, count, train):
    """(mean, invstd) of a channels-last map whose last c - c_real channels are zero padding; in training the running
    statistics of `bn` are updated."""
    c = y.shape[-1]
    rm, rv = pad_c(bn.running_mean, c), pad_c(bn.running_var, c, 1.0)
    if not train:
        return ops.bn_eval_stats(rm, rv, bn.eps)
    mean, invstd = ops.bn_finalize(ops.bn_stats(y, c), count, rm, rv, bn.num_batches_tracked, bn.eps, bn.momentum)
    if c != c_real:
        bn.running_mean.copy_(rm[:c_real])
        bn.running_var.copy_(rv[:c_real])
    return mean, invstd


def bn_eval_reduce(sums):
    """BatchNorm backward for a forward that used RUNNING statistics: mean and variance do not depend on the batch, so
    dy = gamma * invstd * g without the batch-mean terms.  The split backward (ops.bn_pool_act_bwd with `reduce_fn`) takes the
    dx coefficients from this [2C + 1] vector (sum g, sum g * xhat, count) and dgamma / dbeta from the untouched local copy:
    zeroing the two sums is the eval-mode formula."""
    sums[:-1].zero_()
    return sums


def mark_touched(model, grads):
    """tell a FusedAdam built on this model which parameters just received a gradient (torch.optim.Adam skips the rest)"""
    flat = getattr(model, "_maavss_flat", None)
    if flat is not None:
        flat.mark(n for n, g in grads.items() if g is not None)


# ---- BiLSTM (bias-free, hidden 256) over a sequence buffer seq [B, L, feat]; the Linear layers around it are weight-streaming
# (HBM-bound at M = batch) with f32 weights in HBM, so they always use the exact-f32 MFMA
def bilstm_fwd(seq, lstm):
    """-> (av [B,L,512], hp, gs, cs): the two input projections into one gate buffer, then the recurrent kernel."""
    b, l, feat = seq.shape
    seq2d = seq.view(b * l, feat)
    gx = torch.empty(b * l, 2048, device=seq.device, dtype=torch.float32)
    ops.gemm(seq2d, lstm.weight_ih_l0.detach(), out=gx[:, :1024], precise=ops.MODE_F32, split_k=1)
    ops.gemm(seq2d, lstm.weight_ih_l0_reverse.detach(), out=gx[:, 1024:], precise=ops.MODE_F32, split_k=1)
    return ops.lstm_fwd(gx.view(b, l, 2, 4, 256), lstm.weight_hh_l0.detach(), lstm.weight_hh_l0_reverse.detach())


def bilstm_wgrad_operands(dgx, seq, hp):
    """(parameter name, dz, x) of the four LSTM weight gradients dW = dz^T @ x, from the gate gradient dgx [B*L, 2048]"""
    rows = dgx.shape[0]
    seq2d, hp2 = seq.view(rows, -1), hp.view(rows, 512)
    return (("lstm.weight_ih_l0", dgx[:, :1024], seq2d), ("lstm.weight_ih_l0_reverse", dgx[:, 1024:], seq2d),
            ("lstm.weight_hh_l0", dgx[:, :1024], hp2[:, :256]), ("lstm.weight_hh_l0_reverse", dgx[:, 1024:], hp2[:, 256:]))


def bilstm_dseq(dgx, lstm):
    """d(seq) [B*L, feat] from the gate gradient"""
    dseq = ops.gemm(dgx[:, :1024], lstm.weight_ih_l0.detach(), trans_b=True, precise=ops.MODE_F32)
    ops.gemm(dgx[:, 1024:], lstm.weight_ih_l0_reverse.detach(), trans_b=True, out=dseq, beta=1, precise=ops.MODE_F32)
    return dseq
