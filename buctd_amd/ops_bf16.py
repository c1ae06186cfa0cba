"""bf16 inference mode of the HRNet / preNet pose networks (csrc/conv_bf16.hip).

Eval forward only.  Every BatchNorm of the trunk folds into the convolution in front of it, so the network reduces to
conv + bias (+ bf16 residual) (+ ReLU) and the fuse rows.  Activations are bf16 NHWC (torch.bfloat16 tensors), filters
are folded bf16 images [Co][Kp] with an fp32 bias, one bf16 MFMA per product with fp32 accumulation.  The preNet's thin
3-channel and 7x7 convolutions stay on the fp32 engine; its output is rounded to bf16 once, at the stem input.

Nothing in ops.py dispatches here: the mode is reached through engine.Bf16Inference only.
"""
import ctypes as C

import torch

from . import nn
from . import ops
from ._C import check, lib, ptr, stream_ptr
from .models.hrnet_common import BasicBlock, Bottleneck

BF16 = torch.bfloat16


def image_k(Ci, R):
    """K extent of a filter image row: R*R*Ci rounded up to the MFMA K step (32)."""
    return (R * R * Ci + 31) // 32 * 32


def _bf16(t, what):
    if t.dtype != BF16 or not t.is_contiguous():
        raise ValueError(f"{what}: a contiguous torch.bfloat16 tensor is required")
    return t


def from_f32(x):
    """fp32 tensor -> bf16 tensor of the same shape (nearest even)."""
    x = ops._f32(x, "bf16 input")
    y = torch.empty(x.shape, dtype=BF16, device=x.device)
    check(lib().buctd_bf16_from_f32(ptr(x), x.numel(), ptr(y), stream_ptr()), "bf16_from_f32")
    return y


def pack_conv(conv, bn, wimg, bias):
    """Fold `bn` (eval statistics; None: no BatchNorm) and the conv bias into the filter image `wimg` ([Co][Kp] bf16)
    and `bias` ([Co] fp32), in place, on the current stream."""
    w = conv.weight
    Co, Ci, R, S = w.shape
    if R != S:
        raise ValueError("bf16 filter images take square kernels only")
    if wimg.shape != (Co, image_k(Ci, R)) or bias.shape != (Co,):
        raise ValueError("bf16 filter image / bias of the wrong shape")
    _bf16(wimg, "filter image")
    if w.dtype != torch.float32:
        raise ValueError("conv weight: fp32 expected")
    s = w.stride()      # any memory format: the pack kernel reads (co, ci, r, s) through the strides
    if bn is not None:
        g, b, rm, rv = (ops._f32(t, "BatchNorm tensor") for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var))
        eps = float(bn.eps)
    else:
        g = b = rm = rv = None
        eps = 0.0
    check(lib().buctd_bf16_pack_conv(ptr(w), s[0], s[1], s[2], s[3], Co, Ci, R,
                                     ptr(conv.bias), ptr(g), ptr(b), ptr(rm), ptr(rv), eps, ptr(wimg), ptr(bias),
                                     stream_ptr()), "bf16_pack_conv")


def conv(x, wimg, bias, Co, R, stride, pad, residual=None, relu=False, head=False):
    """relu?(conv(x) + bias (+ residual)) on bf16 NHWC x [N][H][W][Ci].  head=False: bf16 NHWC [N][Ho][Wo][Co];
    head=True: fp32 NCHW [N][Co][Ho][Wo] (no residual)."""
    _bf16(x, "bf16 conv input")
    _bf16(wimg, "filter image")
    N, H, W, Ci = x.shape
    if wimg.shape != (Co, image_k(Ci, R)):
        raise ValueError(f"filter image {tuple(wimg.shape)} does not fit Ci={Ci}, Co={Co}, R={R}")
    Ho, Wo = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
    if head:
        y = torch.empty((N, Co, Ho, Wo), dtype=torch.float32, device=x.device)
    else:
        y = torch.empty((N, Ho, Wo, Co), dtype=BF16, device=x.device)
    if residual is not None:
        _bf16(residual, "bf16 residual")
        if tuple(residual.shape) != (N, Ho, Wo, Co):
            raise ValueError("bf16 residual of the wrong shape")
    check(lib().buctd_bf16_conv(ptr(x), N, H, W, Ci, ptr(wimg), ptr(ops._f32(bias, "bias")), Co, R, stride, pad,
                                ptr(residual), int(bool(relu)), int(bool(head)), ptr(y), None, 0, stream_ptr()),
          "bf16_conv")
    return y


def fuse_sum(terms, shifts, relu=True):
    """relu(sum_j upsample_nearest(terms[j], 2^shifts[j])) in bf16 NHWC; fp32 sum in the order of `terms`."""
    if len(terms) != len(shifts) or 0 not in shifts:
        raise ValueError("fuse_sum: one shift per term, one term at the output resolution (shift 0)")
    base = terms[shifts.index(0)]
    N, H, W, Cn = base.shape
    for t, s in zip(terms, shifts):
        _bf16(t, "fuse term")
        if t.device != base.device or tuple(t.shape) != (N, H >> s, W >> s, Cn) or (H >> s) << s != H or (W >> s) << s != W:
            raise ValueError(f"fuse_sum: term {tuple(t.shape)} with shift {s} does not fit the output {(N, H, W, Cn)}")
    out = torch.empty_like(base)
    n = len(terms)
    arr = (C.c_void_p * n)(*[t.data_ptr() for t in terms])
    sh = (C.c_int * n)(*shifts)
    check(lib().buctd_bf16_fuse_sum(arr, sh, n, N, H, W, Cn, int(bool(relu)), ptr(out), stream_ptr()), "bf16_fuse_sum")
    return out


# --------------------------------------------------------------------------------------------------------------------
# the network
# --------------------------------------------------------------------------------------------------------------------
def supported(net):
    """None if `net` can run in bf16, else the reason it cannot."""
    from .models import pose_hrnet, pose_hrnet_coam, transpose_h, pose_resnet
    if isinstance(net, pose_hrnet_coam.PoseHighResolutionNet):
        return "pose_hrnet_coam: its CoAM attention modules have no bf16 kernels yet"
    if isinstance(net, transpose_h.TransPoseH):
        return "transpose_h: its transformer encoder (multi-head attention) has no bf16 kernels yet"
    if isinstance(net, pose_resnet.PoseResNet):
        return "pose_resnet: its deconvolution head has no bf16 kernels yet"
    if type(net) is not pose_hrnet.PoseHighResolutionNet:
        return f"{type(net).__name__}: only models.pose_hrnet networks have a bf16 inference mode"
    return None


class Bf16Net:
    """Folded bf16 filter images of a models.pose_hrnet network and its bf16 eval forward.  The images live in two
    buffers allocated once; repack() rewrites them in place (same addresses), so a captured graph that reads them stays
    valid for as long as this object lives."""

    def __init__(self, net):
        reason = supported(net)
        if reason is not None:
            raise NotImplementedError(f"bf16 inference: {reason}")
        self.net = net
        layers = [(net.conv1, net.bn1), (net.conv2, net.bn2)]
        for m in net.modules():
            if isinstance(m, nn.ConvBN):
                layers.append((m[0], m[1]))
            elif isinstance(m, BasicBlock):
                layers += [(m.conv1, m.bn1), (m.conv2, m.bn2)]
            elif isinstance(m, Bottleneck):
                layers += [(m.conv1, m.bn1), (m.conv2, m.bn2), (m.conv3, m.bn3)]
        layers.append((net.final_layer, None))
        for c, b in layers:
            if b is not None and (b.running_mean is None or b.weight is None):
                raise NotImplementedError("bf16 inference folds affine BatchNorms with running statistics only")
        self.layers = layers
        self.wbuf = self.bbuf = None
        self.img = {}

    def _allocate(self, dev):
        nw = sum(c.out_channels * image_k(c.in_channels, c.kernel_size[0]) for c, _ in self.layers)
        nb = sum(c.out_channels for c, _ in self.layers)
        self.wbuf = torch.empty(nw, dtype=BF16, device=dev)
        self.bbuf = torch.empty(nb, dtype=torch.float32, device=dev)
        ow = ob = 0
        for c, _ in self.layers:
            Co, K = c.out_channels, image_k(c.in_channels, c.kernel_size[0])
            self.img[id(c)] = (self.wbuf[ow:ow + Co * K].view(Co, K), self.bbuf[ob:ob + Co])
            ow += Co * K
            ob += Co

    def repack(self):
        """(Re)build every filter image from the network's current tensors, on the current stream.  The buffers are
        allocated once (again only if the network moved to another device) and rewritten in place."""
        dev = self.net.final_layer.weight.device
        if self.wbuf is None or self.wbuf.device != dev:
            self._allocate(dev)
        for c, b in self.layers:
            wimg, bias = self.img[id(c)]
            pack_conv(c, b, wimg, bias)

    # ---- forward -------------------------------------------------------------------------------------------------
    def _conv(self, c, x, relu=False, residual=None, head=False):
        wimg, bias = self.img[id(c)]
        stride, pad = c._geom()
        return conv(x, wimg, bias, c.out_channels, c.kernel_size[0], stride, pad, residual, relu, head)

    def _convbn(self, m, x, residual=None):
        return self._conv(m[0], x, relu=m._relu, residual=residual)

    def _chain(self, ch, x):
        for m in ch:
            x = self._convbn(m, x)
        return x

    def _block(self, m, x):
        res = x if m.downsample is None else self._convbn(m.downsample, x)
        out = self._conv(m.conv1, x, relu=True)
        if isinstance(m, Bottleneck):
            out = self._conv(m.conv2, out, relu=True)
            return self._conv(m.conv3, out, relu=True, residual=res)
        return self._conv(m.conv2, out, relu=True, residual=res)

    def _blocks(self, chain, x):
        for m in chain:
            x = self._block(m, x)
        return x

    def _hr_module(self, mod, xs):
        ys = [self._blocks(mod.branches[i], xs[i]) for i in range(mod.num_branches)]
        if mod.num_branches == 1:
            return ys
        out = []
        for i, row in enumerate(mod.fuse_layers):
            terms, shifts = [], []
            for j in range(mod.num_branches):
                if j == i:
                    terms.append(ys[j])
                    shifts.append(0)
                elif j > i:
                    terms.append(self._convbn(row[j], ys[j]))   # 1x1 conv + BN at the low resolution
                    shifts.append(j - i)                        # nearest up-sampling while the fuse kernel reads
                else:
                    terms.append(self._chain(row[j], ys[j]))
                    shifts.append(0)
            out.append(fuse_sum(terms, shifts, relu=True))
        return out

    def _enter_stage(self, s, prev, first):
        trans = getattr(self.net, "transition%d" % (s - 1))
        n = getattr(self.net, "stage%d_cfg" % s)["NUM_BRANCHES"]

        def run(t, z):
            return self._convbn(t, z) if isinstance(t, nn.ConvBN) else self._chain(t, z)
        if first:
            return [run(trans[i], prev) if trans[i] is not None else prev for i in range(n)]
        return [run(trans[i], prev[-1]) if trans[i] is not None else prev[i] for i in range(n)]

    def forward(self, x):
        """fp32 NCHW input (CPU or device) -> fp32 NCHW heat-maps."""
        from .models.hrnet_common import to_device_input
        net = self.net
        x = to_device_input(x)
        if net.cfg.MODEL.EXTRA.USE_PRE_NET:
            if x.shape[1] - 3 <= 0:
                raise Exception("condition is empty, please check your dataloader")
            # the preNet on the fp32 engine (thin 3-channel and 7x7 convolutions), exactly as the wrapped network runs it
            rgb = ops.nchw_to_nhwc(x, 0, 3)
            cond = ops.nchw_to_nhwc(x, 3, x.shape[1] - 3)
            r, c = net.rgb_preNet, net.cond_preNet
            x0 = nn.conv_bn_act(rgb, r[0], r[1])
            x0 = nn.conv_bn_act(x0, r[2], r[3])
            xin = nn.conv_bn_act(cond, c[0], c[1], residual=x0)
        else:
            xin = ops.nchw_to_nhwc(x, 0, 3) if x.shape[1] != 3 else ops.nchw_to_nhwc(x)
        h = from_f32(xin)
        h = self._conv(net.conv1, h, relu=True)
        h = self._conv(net.conv2, h, relu=True)
        h = self._blocks(net.layer1, h)
        y = self._enter_stage(2, h, True)
        s = 2
        while hasattr(net, "stage%d" % s):
            if s > 2:
                y = self._enter_stage(s, y, False)
            for mod in getattr(net, "stage%d" % s):
                y = self._hr_module(mod, y)
            s += 1
        return self._conv(net.final_layer, y[0], head=True)
