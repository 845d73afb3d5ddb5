"""Engine pieces that AV_Fusion_Model_Frames (avse.py) and AV_Fusion_Model (avfm.py) both use: the channel-padded
BatchNorm2d glue, the 2-D convolution stacks (conv -> BatchNorm -> tanh per layer, forward and backward) and the BiLSTM
block.  Plain functions over maavss_amd.ops; the heads and the fusion block (_fusion_fwd / _fusion_bwd) stay in the models'
own files: there the two differ in what they compute (tanh / sigmoid without bias against bias + LeakyReLU, hence also in
the bias gradients), not in how it is written."""
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


def bn_train_stats(part, count, bn, sync, rm=None, rv=None):
    """training-mode (mean, invstd) from the partial sums; `sync` (set_bn_sync) all-reduces them over the data-parallel ranks.
    Updates the running statistics rm / rv (default: those of `bn`)."""
    rm, rv = bn.running_mean if rm is None else rm, bn.running_var if rv is None else rv
    if sync is None:
        return ops.bn_finalize(part, count, rm, rv, bn.num_batches_tracked, bn.eps, bn.momentum)
    return ops.bn_finalize_synced(part, count, sync, rm, rv, bn.num_batches_tracked, bn.eps, bn.momentum)


def bn_stats_padded(y, bn, c_real, count, train, sync=None):
    """(mean, invstd) of a channels-last map whose last c - c_real channels are zero padding; in training the running
    statistics of `bn` are updated."""
    c = y.shape[-1]
    rm, rv = pad_c(bn.running_mean, c), pad_c(bn.running_var, c, 1.0)
    if not train:
        return ops.bn_eval_stats(rm, rv, bn.eps)
    mean, invstd = bn_train_stats(ops.bn_stats(y, c), count, bn, sync, rm, rv)
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


def bn_grad_bufs(prefix, idx, need, gbuf, out_grads):
    """(dgamma buffer, dbeta buffer, accumulate) of BatchNorm module `prefix.idx`, entered in out_grads -- or (None, None, False)"""
    nw, nb = f"{prefix}.{idx}.weight", f"{prefix}.{idx}.bias"
    if not (need.get(nw, False) or need.get(nb, False)):
        return None, None, False
    gw, beta = gbuf(nw)
    gb, _ = gbuf(nb)
    out_grads[nw], out_grads[nb] = gw, gb
    return gw, gb, bool(beta)


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


# ---- 2-D convolution stacks: Conv2d / ConvTranspose2d (bias or none) -> BatchNorm2d -> Tanh per layer, the last layer of a
# decoder without the BatchNorm.  All of them run through the generic convolution entry points (ops.conv_gen_*), which pick
# the kernel from the call; maps are ops.Map, channels-last (padded to cpad(c) channels where a BatchNorm follows) or NCHW.
def stack_layers(seq, prefix, kind, strides, pads, bns):
    """resolved layers of the stack held in the nn.Sequential `seq` = model.<prefix>: per layer the conv module, its BatchNorm2d
    or None, kind "conv" / "convT", stride, pad and the module index behind the parameter names `prefix.idx.*`"""
    layers, idx = [], 0
    for st, pd, bn in zip(strides, pads, bns):
        layers.append(dict(conv=seq[idx], bn=seq[idx + 1] if bn else None, kind=kind, stride=tuple(st), pad=tuple(pd), prefix=prefix, idx=idx))
        idx += 3 if bn else 1
    return layers


def stack_forward(layers, x_map, train, bn_sync=None, final_nchw=False, seq_out=None):
    """x_map: ops.Map of the input.  Runs conv(+bias) -> BN -> tanh per layer.  `seq_out` = (flat buffer, strides) makes the last
    layer's BN + tanh write there (the LSTM sequence buffer; strides (batch, row, column, channel)), `final_nchw` a last layer
    without BatchNorm write the network's NCHW output, `bn_sync` (set_bn_sync) all-reduces the training statistics.
    Returns (ops.Map of the output, or None with seq_out; saved records, one per layer)."""
    saved, cur, b = [], x_map, x_map.b
    for li, layer in enumerate(layers):
        conv, bn, st, pd = layer["conv"], layer["bn"], layer["stride"], layer["pad"]
        w, bias = conv.weight.detach(), None if conv.bias is None else conv.bias.detach()
        kh, kw = w.shape[2], w.shape[3]
        if layer["kind"] == "conv":
            co = w.shape[0]
            ho, wo = (cur.h + 2 * pd[0] - kh) // st[0] + 1, (cur.w + 2 * pd[1] - kw) // st[1] + 1
        else:
            co, op = w.shape[1], conv.output_padding
            ho, wo = (cur.h - 1) * st[0] - 2 * pd[0] + kh + op[0], (cur.w - 1) * st[1] - 2 * pd[1] + kw + op[1]
        if bn is None and final_nchw:
            ymap = ops.Map(torch.empty(b, co, ho, wo, device=cur.t.device, dtype=torch.float32), nchw=True)
        else:       # channels-last, padded to what the BatchNorm kernels take: the dead channels must be (and stay) exactly zero
            cp = cpad(co) if bn is not None else co
            y = (torch.zeros if cp != co else torch.empty)(b, ho, wo, cp, device=cur.t.device, dtype=torch.float32)
            ymap = ops.Map(y, c=co)
        (ops.conv_gen_small if layer["kind"] == "conv" else ops.conv_gen_big)(cur, w, bias, ymap, st, pd)
        rec = dict(x=cur, y=ymap, hw=(ho, wo))
        if bn is not None:
            mean, invstd = bn_stats_padded(y, bn, co, b * ho * wo, train, bn_sync)
            gamma, beta = pad_c(bn.weight.detach(), cp), pad_c(bn.bias.detach(), cp)
            # the BatchNorm kernels index pooled positions flat, so any split of the rows over their "T" and "H" addresses the same
            # elements in the same order; here "T" = the map's rows, one spatial row each: strides per row / column
            y5 = y.view(b, ho, 1, wo, cp)
            buf, strides = seq_out if seq_out is not None and li == len(layers) - 1 else (None, None)
            assert strides is None or cp == co
            out, _ = ops.bn_pool_act_fwd(y5, mean, invstd, gamma, beta, 1, ops.BN_TANH, out=buf, strides=strides)
            rec.update(y5=y5, mean=mean, invstd=invstd, gamma=gamma, out=out, strides=strides)
            cur = ops.Map(out.view(b, ho, wo, cp), c=co) if strides is None else None
        else:
            cur = ymap
        saved.append(rec)
    return cur, saved


def stack_backward(layers, saved, dout, need, gbuf, out_grads, out=None, bn_reduce=None, want_dx=False):
    """Backward of stack_forward.  dout: gradient w.r.t. the stack's output, shaped like it (channels-last padded / NCHW) -- or, with
    `out`, gradient and value of an output that lives in the LSTM sequence buffer, as flat views from its first element.
    `need[name]` says which parameter gradients are wanted, `gbuf(name)` -> (buffer, beta) gives where they go (beta = 1: added to
    what the buffer holds); results are entered in out_grads.  `bn_reduce`: ops.bn_pool_act_bwd's reduce_fn (the eval-mode backward
    bn_eval_reduce, or the all-reduce of set_bn_sync).  Returns the gradient w.r.t. the input (a tensor laid out like it) if
    `want_dx`, else None."""
    dx = None
    for li in reversed(range(len(layers))):
        layer, s = layers[li], saved[li]
        conv, st, pd, prefix, idx = layer["conv"], layer["stride"], layer["pad"], layer["prefix"], layer["idx"]
        w, ymap = conv.weight.detach(), s["y"]
        if layer["bn"] is not None:
            c, cp = ymap.c, ymap.c_alloc
            if s["strides"] is None:
                dout, out = dout.view(s["y5"].shape), s["out"]
            if cp == c:     # straight into the sink
                gw, gb, acc = bn_grad_bufs(prefix, idx + 1, need, gbuf, out_grads)
            else:           # channel-padded: through a temporary and a slice
                gw, gb, acc = torch.empty_like(s["gamma"]), torch.empty_like(s["gamma"]), False
            dy = ops.bn_pool_act_bwd(dout, out, None, s["y5"], s["mean"], s["invstd"], s["gamma"], 1, ops.BN_TANH, strides=s["strides"],
                                     dgamma=gw, dbeta=gb, accumulate=acc, reduce_fn=bn_reduce)
            if cp != c:
                for name, g in ((f"{prefix}.{idx + 1}.weight", gw), (f"{prefix}.{idx + 1}.bias", gb)):
                    if need.get(name, False):
                        buf, beta = gbuf(name)
                        out_grads[name] = buf.add_(g[:c]) if beta else buf.copy_(g[:c])
            dymap = ops.Map(dy.view(ymap.t.shape), c=c)
        else:
            dymap = ops.Map(dout, nchw=ymap.nchw, c=ymap.c)
        small, big = (dymap, s["x"]) if layer["kind"] == "conv" else (s["x"], dymap)
        if need.get(f"{prefix}.{idx}.bias", False):
            buf, beta = gbuf(f"{prefix}.{idx}.bias")
            out_grads[f"{prefix}.{idx}.bias"] = ops.channel_sum(dymap, out=buf, beta=beta)
        if need.get(f"{prefix}.{idx}.weight", False):
            buf, beta = gbuf(f"{prefix}.{idx}.weight")
            out_grads[f"{prefix}.{idx}.weight"] = ops.conv_gen_wgrad(small, big, w.shape, st, pd, dw=buf, beta=beta)
        if li > 0 or want_dx:
            xm = s["x"]
            dx = (torch.zeros_like if xm.c != xm.c_alloc else torch.empty_like)(xm.t)
            dxm = ops.Map(dx, nchw=xm.nchw, c=xm.c)
            if layer["kind"] == "conv":
                ops.conv_gen_big(dymap, w, None, dxm, st, pd)
            else:
                ops.conv_gen_small(dymap, w, None, dxm, st, pd)
            dout, out = dx, None
    return dx if want_dx else None
