"""Autograd Functions of the TransPose encoder and the ResNet stem on top of buctd_amd.ops:
LayerNorm, element-wise dropout, position-embedding add, channel concat, max-pool, and the
nn.MultiheadAttention input projection (reference lib/models/transpose_h.py:168-243, 668-681;
lib/models/pose_resnet.py:122).  Every numeric step is a libbuctd_hip.so kernel."""
import ctypes as C

import torch

from . import ops
from ._C import check, lib, ptr, stream_ptr


def copy_channels(src, cs0, dst, cd0, cc):
    rows = src.numel() // src.shape[-1]
    check(lib().buctd_copy_channels(ptr(src), rows, src.shape[-1], cs0, ptr(dst), dst.shape[-1], cd0, cc, stream_ptr()),
          "copy_channels")


def add_bcast(a, v):
    out = torch.empty_like(a)
    n = v.numel()
    check(lib().buctd_add_bcast(ptr(a), ptr(v), ptr(out), a.numel() // n, n, stream_ptr()), "add_bcast")
    return out


class ConcatChannels(torch.autograd.Function):
    """torch.cat((a, b), dim=channel) on NHWC tensors."""

    @staticmethod
    def forward(ctx, a, b):
        ca, cb = a.shape[-1], b.shape[-1]
        out = torch.empty(a.shape[:-1] + (ca + cb,), dtype=torch.float32, device=a.device)
        copy_channels(a, 0, out, 0, ca)
        copy_channels(b, 0, out, ca, cb)
        ctx.dims = (tuple(a.shape), tuple(b.shape))
        return out

    @staticmethod
    def backward(ctx, dy):
        sa, sb = ctx.dims
        dy = dy.contiguous()
        da = db = None
        if ctx.needs_input_grad[0]:
            da = torch.empty(sa, dtype=torch.float32, device=dy.device)
            copy_channels(dy, 0, da, 0, sa[-1])
        if ctx.needs_input_grad[1]:
            db = torch.empty(sb, dtype=torch.float32, device=dy.device)
            copy_channels(dy, sa[-1], db, 0, sb[-1])
        return da, db


def batch_sum(x, out, accumulate):
    """out (+)= x summed over its leading (batch) dimension, rows added in ascending order"""
    n = out.numel()
    check(lib().buctd_batch_sum(ptr(x), x.numel() // n, n, ptr(out), int(accumulate), stream_ptr()), "batch_sum")


class _PosUses:
    """The AddPos nodes of one forward pass that owe a trainable embedding a gradient piece."""

    def __init__(self):
        self.nodes = 0      # AddPos nodes of the pass
        self.done = 0       # ... that have added their piece in the backward under way


class AddPos(torch.autograd.Function):
    """tokens [B,T,d] + pos (T*d values: [T,d] or the reference's [T,1,d] parameter, transpose_h.py:494-511).

    The sine embedding is a constant and takes no gradient.  A learnable one (`pos` is the parameter itself, or a view of
    it) is added in every encoder layer, so its gradient is a sum over layers and images.  It goes through the
    parameter-gradient sink like every other one: each node's backward adds its batch sum to ops.grad_target(param) - the
    first piece of a backward overwrites or accumulates as grad_target says, the later ones accumulate - and the node that
    adds the last piece of its forward pass (layer 0's: backward runs the layers in reverse) calls ops.grad_done(param),
    once.  The pieces are counted per forward pass: forward() joins the parameter's open count when it will need the
    gradient (add_pos() keeps no_grad forwards out), begin() (the encoder's forward) and the first backward of a pass
    close it, so a forward that is never backpropagated leaves nothing behind.  A further backward through a retained graph
    adds and reports again; one backward through two forward passes of the same parameter reports it twice.
    engine.DataParallel answers both like any second write to a counted gradient."""

    @staticmethod
    def begin(pos):
        """a new forward pass starts: the AddPos nodes that follow are counted on their own"""
        if pos is not None and pos.requires_grad:
            _pos_param(pos)._pos_uses = None

    @staticmethod
    def forward(ctx, x, pos):
        ctx.uses = None
        if ctx.needs_input_grad[1]:
            param = _pos_param(pos)
            if not (param.is_leaf and param.is_contiguous() and param.numel() == pos.numel()
                    and param.data_ptr() == pos.data_ptr() and pos.is_contiguous()):
                raise ValueError("AddPos: a trainable position embedding is the parameter itself or a contiguous view of "
                                 "all of it")
            uses = getattr(param, "_pos_uses", None)
            if uses is None:
                uses = param._pos_uses = _PosUses()
            uses.nodes += 1
            ctx.param, ctx.uses = param, uses
        return add_bcast(x, pos)

    @staticmethod
    def backward(ctx, dy):
        uses = ctx.uses
        if uses is None:
            return dy, None
        param = ctx.param
        if getattr(param, "_pos_uses", None) is uses:
            param._pos_uses = None              # this pass is being backpropagated: the next forward counts anew
        g, acc = ops.grad_target(param)
        batch_sum(dy.contiguous(), g, acc)
        uses.done += 1
        if uses.done == uses.nodes:
            uses.done = 0                       # a second backward through a retained graph is counted, and reported, again
            ops.grad_done(param)
        return dy, None


def _pos_param(pos):
    return pos if pos._base is None else pos._base


def add_pos(x, pos):
    """AddPos as the modules call it: under no_grad a trainable embedding is a constant (a Function's forward cannot tell,
    it always runs with gradients off) and is not counted"""
    if pos.requires_grad and not torch.is_grad_enabled():
        pos = pos.detach()
    return AddPos.apply(x, pos)


class Dropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, training):
        if not training or p == 0.0:
            ctx.seed = None
            return x
        ctx.seed, ctx.p = ops.next_seed(), p
        return ops.dropout(x.contiguous(), p, ctx.seed)

    @staticmethod
    def backward(ctx, dy):
        if ctx.seed is None:
            return dy, None, None
        return ops.dropout(dy.contiguous(), ctx.p, ctx.seed), None, None  # same mask, same 1/(1-p) scale


class AddLayerNorm(torch.autograd.Function):
    """LayerNorm(a + b) with affine parameters (post-norm residual, transpose_h.py:204-209)."""

    @staticmethod
    def forward(ctx, a, b, ln, anchor=None):
        # anchor (ops.grad_anchor): builds the node for ln's parameters, which autograd does not see
        keep = any(ctx.needs_input_grad)     # backward() runs only then (it also owns ln's gradients)
        y, mean, invstd, s = ops.add_layernorm_fwd(a.contiguous(), b.contiguous(), ln.weight, ln.bias, ln.eps, keep_sum=keep)
        ctx.ln = ln
        if keep:
            ctx.save_for_backward(s, mean, invstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        s, mean, invstd = ctx.saved_tensors
        ln = ctx.ln
        dg, acc = ops.grad_target(ln.weight)
        db, acc2 = ops.grad_target(ln.bias)
        acc = ops.norm_acc(ln.weight, acc, ln.bias, acc2)
        ds = ops.layernorm_bwd(dy.contiguous(), s, mean, invstd, ln.weight, dg, db, acc)
        ops.grad_done(ln.weight, ln.bias)
        return ds, ds, None, None


class InProjection(torch.autograd.Function):
    """nn.MultiheadAttention input projection with q = k = src + pos and v = src:
    qk = (src+pos) W[:2d]^T + b[:2d],  v = src W[2d:]^T + b[2d:]  (transpose_h.py:192-197)."""

    @staticmethod
    def forward(ctx, qin, src, w, b):
        d = w.shape[1]
        B, T, _ = src.shape
        qk = ops.conv_fwd(qin.view(B, 1, T, d), w[: 2 * d], b[: 2 * d], 1, 0)
        v = ops.conv_fwd(src.view(B, 1, T, d), w[2 * d:], b[2 * d:], 1, 0)
        ctx.pw, ctx.pb = w, b
        ctx.save_for_backward(qin, src)
        return qk.view(B, T, 2 * d), v.view(B, T, d)

    @staticmethod
    def backward(ctx, dqk, dv):
        qin, src = ctx.saved_tensors
        w, b = ctx.pw, ctx.pb
        d = w.shape[1]
        B, T, _ = src.shape
        dqk = dqk.contiguous().view(B, 1, T, 2 * d)
        dv = dv.contiguous().view(B, 1, T, d)
        x4 = (B, 1, T, d)
        dqin = ops.conv_dgrad(dqk, w[: 2 * d], x4, 1, 0).view(B, T, d)
        dsrc = ops.conv_dgrad(dv, w[2 * d:], x4, 1, 0).view(B, T, d)
        if w.requires_grad:
            gw, acc = ops.grad_target(w)
            ops.conv_wgrad(qin.view(x4), dqk, w[: 2 * d], 1, 0, out=gw[: 2 * d], accumulate=acc)
            ops.conv_wgrad(src.view(x4), dv, w[2 * d:], 1, 0, out=gw[2 * d:], accumulate=acc)
        if b.requires_grad:
            gb, accb = ops.grad_target(b)
            ops.colsum(dqk, 2 * d, gb[: 2 * d], accb)
            ops.colsum(dv, d, gb[2 * d:], accb)
        ops.grad_done(w, b)
        return dqin, dsrc, None, None


class MaxPool3x3s2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        y, idx = ops.maxpool3x3s2_fwd(x)
        ctx.save_for_backward(idx)
        ctx.xshape = tuple(x.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        return ops.maxpool3x3s2_bwd(dy.contiguous(), idx, ctx.xshape)
