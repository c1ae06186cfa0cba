"""bf16 inference mode (engine.Bf16Inference, buctd_amd/ops_bf16.py, csrc/conv_bf16.hip) on the MI355X.

Kernel exactness is checked against an fp64 torch evaluation of the SAME bf16-rounded operands and folded bias, so
the only error left is the fp32 accumulation order (plus the one bf16 rounding of a bf16 output).  Whole networks are
checked against the committed fp32 goldens of the reference with the accuracy bound of DESIGN.md 8: relative heat-map
error and arg-max agreement, never in place of the 1e-3 fp32 check the default mode passes.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BF16 = torch.bfloat16

# whole-network bounds (measured on the MI355X; each is 2x the measured value, clamped to the floors
# rel L2 <= 3e-2, agreement >= 90 %, every disagreement <= 1 heat-map pixel)
NET_BOUNDS = {
    "prenet_w16_96x64": {"rel_l2": 3e-2, "rel_max": 6e-2, "agree": 0.90},
    "prenet_w32_256x192": {"rel_l2": 3e-2, "rel_max": 6e-2, "agree": 0.90},
}


def _bf16_ref_bound(ref, out_bf16):
    """1e-5 * (max|ref| + 1) for fp32 accumulation order, plus one bf16 rounding of the result for a bf16 output."""
    tol = 1e-5 * (float(ref.abs().max()) + 1.0)
    return tol + (ref.abs() * 2.0 ** -8 if out_bf16 else 0.0)


def _random_conv_bn(Ci, Co, R, stride, seed, conv_bias=False, bn=True):
    from buctd_amd import nn
    g = torch.Generator().manual_seed(seed)
    conv = nn.Conv2d(Ci, Co, R, stride, R // 2, bias=conv_bias)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / (R * R * Ci) ** 0.5)
        if conv_bias:
            conv.bias.copy_(torch.randn(Co, generator=g) * 0.1)
    b = None
    if bn:
        b = nn.BatchNorm2d(Co)
        with torch.no_grad():
            b.weight.copy_(torch.rand(Co, generator=g) + 0.5)
            b.bias.copy_(torch.randn(Co, generator=g) * 0.2)
            b.running_mean.copy_(torch.randn(Co, generator=g) * 0.3)
            b.running_var.copy_(torch.rand(Co, generator=g) + 0.25)
        b.eval()
    return conv, b


def _packed(conv, bn, dev):
    from buctd_amd import ops_bf16
    Co, Ci, R, _ = conv.weight.shape
    conv = conv.to(dev)
    bn = bn.to(dev) if bn is not None else None
    wimg = torch.empty(Co, ops_bf16.image_k(Ci, R), dtype=BF16, device=dev)
    bias = torch.empty(Co, dtype=torch.float32, device=dev)
    ops_bf16.pack_conv(conv, bn, wimg, bias)
    return conv, bn, wimg, bias


def _host_fold(conv, bn):
    """host fold (scale in fp64 rounded to fp32, the rest in fp32), then one torch.bfloat16 rounding: the pack kernel's
    contract."""
    w = conv.weight.detach().float().cpu()
    cb = conv.bias.detach().float().cpu() if conv.bias is not None else torch.zeros(w.shape[0])
    if bn is None:
        return w.to(BF16), cb
    g, b = bn.weight.detach().cpu(), bn.bias.detach().cpu()
    m, v = bn.running_mean.cpu(), bn.running_var.cpu()
    eps = torch.tensor(bn.eps, dtype=torch.float32).double()
    scale = (g.double() / torch.sqrt(v.double() + eps)).float()
    return (w * scale.view(-1, 1, 1, 1)).to(BF16), (cb - m) * scale + b


def _image_as_oihw(wimg, Ci, R):
    Co = wimg.shape[0]
    return wimg[:, :R * R * Ci].reshape(Co, R, R, Ci).permute(0, 3, 1, 2)


# (R, stride, Ci, Co, N, H, W, residual, relu, head)
CONV_CASES = [
    (3, 1, 32, 32, 1, 24, 18, True, True, False),
    (3, 1, 48, 48, 3, 12, 9, True, True, False),
    (3, 1, 96, 96, 1, 8, 6, False, True, False),
    (3, 1, 384, 384, 1, 12, 9, True, True, False),
    (3, 1, 192, 128, 3, 9, 7, False, False, False),
    (3, 1, 256, 48, 1, 16, 12, False, True, False),
    (3, 2, 3, 64, 3, 37, 29, False, True, False),
    (3, 2, 64, 64, 1, 48, 36, False, True, False),
    (3, 2, 96, 192, 3, 24, 18, False, False, False),
    (3, 2, 48, 384, 1, 13, 9, False, False, False),
    (1, 1, 64, 256, 3, 24, 18, True, True, False),
    (1, 1, 192, 48, 1, 12, 9, False, False, False),
    (1, 1, 384, 32, 3, 3, 5, False, False, False),
    (1, 1, 32, 3, 1, 8, 6, False, False, True),
    (1, 1, 48, 192, 3, 24, 18, False, False, True),
    (3, 1, 64, 96, 1, 12, 9, False, True, True),
]


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "r{}s{}_ci{}_co{}_n{}_{}x{}{}{}{}".format(
    c[0], c[1], c[2], c[3], c[4], c[5], c[6], "_res" if c[7] else "", "_relu" if c[8] else "", "_f32" if c[9] else ""))
def test_bf16_conv_matches_fp64_on_the_same_bf16_operands(dev, case):
    from buctd_amd import ops_bf16
    R, stride, Ci, Co, N, H, W, res, relu, head = case
    conv, bn = _random_conv_bn(Ci, Co, R, stride, seed=Ci * 1000 + Co + R + stride)
    conv, bn, wimg, bias = _packed(conv, bn, dev)
    g = torch.Generator().manual_seed(N * 100 + H)
    x = torch.randn(N, H, W, Ci, generator=g).to(BF16).to(dev)
    pad = R // 2
    Ho, Wo = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
    r = torch.randn(N, Ho, Wo, Co, generator=g).to(BF16).to(dev) if res else None
    y = ops_bf16.conv(x, wimg, bias, Co, R, stride, pad, residual=r, relu=relu, head=head)
    torch.cuda.synchronize()
    w64 = _image_as_oihw(wimg, Ci, R).double().cpu()
    ref = F.conv2d(x.double().cpu().permute(0, 3, 1, 2), w64, bias.double().cpu(), stride, pad)
    if r is not None:
        ref = ref + r.double().cpu().permute(0, 3, 1, 2)
    if relu:
        ref = ref.clamp_min(0)
    got = y.double().cpu() if head else y.double().cpu().permute(0, 3, 1, 2)
    assert got.shape == ref.shape
    err = (got - ref).abs()
    bound = _bf16_ref_bound(ref, not head)
    assert bool((err <= bound).all()), f"max |d| {float(err.max()):.3e}, max|ref| {float(ref.abs().max()):.3e}"


def _tile_mt(M, Co):
    """The pixel tile (MT) buctd_bf16_conv picks: the largest of 4 / 2 / 1 that still gives >= 1024 blocks."""
    nt = 2 if Co <= 32 else 3 if (Co % 64 != 0 and Co % 48 == 0) else 4
    nn_ = -(-Co // (16 * nt))
    return 4 if -(-M // 256) * nn_ >= 1024 else 2 if -(-M // 128) * nn_ >= 1024 else 1


def _large_cases():
    """The MT = 2 / MT = 4 tiles of every channel tile (NT 2 / 3 / 4) of both the vector (Ci % 8 == 0) and the gather paths:
    the small-operand cases of tests/helpers/bf16_cases.py (Ci <= 17, the smallest M that meets the block threshold), as
    (case of this file, MT, instance name)."""
    from tests.helpers import bf16_cases as B
    out = []
    for c in B.CONV_LARGE:
        R, stride, pad, Ci, Co, N, H, W, res, relu, head = c
        assert pad == R // 2
        mt, nt, vec = B.conv_instance(c)
        out.append(((R, stride, Ci, Co, N, H, W, bool(res), bool(relu), bool(head)), mt, B.inst_name(mt, nt, vec)[5:]))
    return out


LARGE_CASES = _large_cases()


def test_large_cases_name_every_large_tile_instance():
    assert sorted(n for _, _, n in LARGE_CASES) == sorted(
        f"MT{mt}-NT{nt}-{v}" for mt in (2, 4) for nt in (2, 3, 4) for v in ("vec", "gather"))


@pytest.mark.parametrize("case,mt,inst", LARGE_CASES, ids=[n for _, _, n in LARGE_CASES])
def test_bf16_conv_large_tiles_match_fp64(dev, case, mt, inst):
    R, stride, Ci, Co, N, H, W = case[:7]
    Ho, Wo = (H + 2 * (R // 2) - R) // stride + 1, (W + 2 * (R // 2) - R) // stride + 1
    assert _tile_mt(N * Ho * Wo, Co) == mt, "the case no longer selects the tile it is meant to cover"
    nt = 2 if Co <= 32 else 3 if (Co % 64 != 0 and Co % 48 == 0) else 4
    assert inst == f"MT{mt}-NT{nt}-{'vec' if Ci % 8 == 0 else 'gather'}"
    test_bf16_conv_matches_fp64_on_the_same_bf16_operands(dev, case)


@pytest.mark.parametrize("Ci,Co,R,conv_bias,bn,channels_last", [
    (3, 64, 3, False, True, False), (64, 256, 1, False, True, True), (48, 96, 3, False, True, True),
    (32, 17, 1, True, False, False), (3, 3, 3, True, True, True)])
def test_bf16_weight_pack_is_bit_identical_to_a_host_fold(dev, Ci, Co, R, conv_bias, bn, channels_last):
    conv, b = _random_conv_bn(Ci, Co, R, 1, seed=Ci + 7 * Co, conv_bias=conv_bias, bn=bn)
    if channels_last:
        conv.weight.data = conv.weight.data.contiguous(memory_format=torch.channels_last)
    w_ref, b_ref = _host_fold(conv, b)
    conv, b, wimg, bias = _packed(conv, b, dev)
    torch.cuda.synchronize()
    img = wimg.cpu()
    assert torch.equal(_image_as_oihw(img, Ci, R).view(torch.int16), w_ref.view(torch.int16))
    assert not img[:, R * R * Ci:].view(torch.int16).any(), "K padding of the image must be zero"
    assert torch.equal(bias.cpu(), b_ref)


@pytest.mark.parametrize("C,shifts,N,H,W", [(32, (0, 1, 2, 3), 3, 64, 48), (96, (2, 1, 0), 1, 24, 16),
                                            (48, (0, 1), 3, 12, 8), (384, (0,), 1, 8, 6)])
def test_bf16_fuse_row_matches_torch_restatement(dev, C, shifts, N, H, W):
    from buctd_amd import ops_bf16
    g = torch.Generator().manual_seed(C + N)
    terms = [torch.randn(N, H >> s, W >> s, C, generator=g).to(BF16).to(dev) for s in shifts]
    y = ops_bf16.fuse_sum(terms, list(shifts), relu=True)
    torch.cuda.synchronize()
    ref = torch.zeros(N, H, W, C, dtype=torch.float64)
    for t, s in zip(terms, shifts):
        ref += t.double().cpu().repeat_interleave(1 << s, 1).repeat_interleave(1 << s, 2)
    ref = ref.clamp_min(0)
    err = (y.double().cpu() - ref).abs()
    assert bool((err <= _bf16_ref_bound(ref, True)).all()), float(err.max())


# ---- whole networks ---------------------------------------------------------------------------------------------------
def _product(name, dev):
    from oracle import recipes
    from buctd_amd import models
    cfg, omodel, x, _ = recipes.build(name)
    net = models.pose_hrnet.get_pose_net(cfg, is_train=False)
    net.load_state_dict(omodel.state_dict(), strict=True)
    return cfg, net.to(dev).eval(), x


def heatmap_metrics(y, ref):
    """-> relative L2, max|d| / max|ref|, arg-max agreement rate, Chebyshev pixel distance of every disagreement."""
    y, ref = np.asarray(y, np.float64), np.asarray(ref, np.float64)
    rel_l2 = float(np.linalg.norm(y - ref) / np.linalg.norm(ref))
    rel_max = float(np.abs(y - ref).max() / np.abs(ref).max())
    Wd = ref.shape[3]
    a = y.reshape(y.shape[0], y.shape[1], -1).argmax(2)
    b = ref.reshape(ref.shape[0], ref.shape[1], -1).argmax(2)
    agree = float((a == b).mean())
    dist = np.maximum(np.abs(a // Wd - b // Wd), np.abs(a % Wd - b % Wd))[a != b]
    return rel_l2, rel_max, agree, dist


def _rb(t):
    """fp64 -> fp32 -> bf16 -> fp64: the kernels' fp32 result rounded once to bf16 storage."""
    return t.float().to(BF16).double()


class Restated(torch.nn.Module):
    """Independent fp64 torch restatement of the bf16 forward of a pose_hrnet network, on the CPU, written against the
    network's module structure (reference HRNet order): the wrapper's folded bf16 images and fp32 biases, each
    convolution's conv + bias (+ residual) (+ ReLU) rounded to bf16, fuse rows summed then rounded, the preNet in
    fp64 with its eval BatchNorms and its output rounded to bf16 at the stem input, the head kept in fp32."""

    def __init__(self, wrap, record=None):
        super().__init__()
        self.wrap = wrap
        self.training = False
        # teacher forcing: `record` holds what the wrapper's kernels produced in one forward ("conv": filter-image
        # address -> output, "fuse" / "stem": outputs in call order).  Each step is then computed from the wrapper's
        # own inputs, checked against the kernel's output, and the kernel's output is passed on: a wiring error shows
        # at the step where it happens, while the chaotic growth of rounding differences is cut at every step
        self.record, self.worst = record, []

    def _out(self, y, head, rec, what):
        if self.record is None:
            return y.float().double() if head else _rb(y)
        got = rec.double().cpu() if head else rec.double().cpu().permute(0, 3, 1, 2)
        if got.shape != y.shape:
            raise AssertionError(f"{what}: wrapper output {tuple(got.shape)}, restatement {tuple(y.shape)}")
        err = (got - y).abs()
        bound = _bf16_ref_bound(y, not head)
        self.worst.append((what, float((err / bound).max())))
        return got

    def _conv(self, c, x, relu=False, res=None, head=False):
        wimg, bias = self.wrap._net.img[id(c)]
        w = _image_as_oihw(wimg.cpu(), c.in_channels, c.kernel_size[0]).double()
        y = F.conv2d(x, w, bias.cpu().double(), c.stride, c.padding)
        if res is not None:
            y = y + res
        if relu:
            y = y.clamp_min(0)
        rec = self.record["conv"][wimg.data_ptr()] if self.record is not None else None
        return self._out(y, head, rec, f"conv {tuple(c.weight.shape)}")

    def _convbn(self, m, x):
        return self._conv(m[0], x, relu=m._relu)

    def _block(self, m, x):
        from buctd_amd.models.hrnet_common import Bottleneck
        res = x if m.downsample is None else self._convbn(m.downsample, x)
        o = self._conv(m.conv1, x, relu=True)
        if isinstance(m, Bottleneck):
            o = self._conv(m.conv2, o, relu=True)
            return self._conv(m.conv3, o, relu=True, res=res)
        return self._conv(m.conv2, o, relu=True, res=res)

    def _module(self, mod, xs):
        ys = []
        for i in range(mod.num_branches):
            y = xs[i]
            for m in mod.branches[i]:
                y = self._block(m, y)
            ys.append(y)
        if mod.num_branches == 1:
            return ys
        out = []
        for i, row in enumerate(mod.fuse_layers):
            acc = None
            for j in range(mod.num_branches):
                if j == i:
                    t = ys[j]
                elif j > i:
                    f = 2 ** (j - i)
                    t = self._convbn(row[j], ys[j]).repeat_interleave(f, 2).repeat_interleave(f, 3)
                else:
                    t = ys[j]
                    for m in row[j]:
                        t = self._convbn(m, t)
                acc = t if acc is None else acc + t
            rec = self.record["fuse"].pop(0) if self.record is not None else None
            out.append(self._out(acc.clamp_min(0), False, rec, f"fuse row {i}"))
        return out

    def _trans(self, t, z):
        from buctd_amd import nn
        if isinstance(t, nn.ConvBN):
            return self._convbn(t, z)
        for m in t:
            z = self._convbn(m, z)
        return z

    @staticmethod
    def _cbn(conv, bn, x):
        p = (conv.kernel_size[0] - 1) // 2
        y = F.conv2d(x, conv.weight.detach().cpu().double(), None if conv.bias is None else conv.bias.detach().cpu().double(),
                     1, p)
        return F.batch_norm(y, bn.running_mean.cpu().double(), bn.running_var.cpu().double(),
                            bn.weight.detach().cpu().double(), bn.bias.detach().cpu().double(), False, 0.0, bn.eps)

    def forward(self, x):
        net = self.wrap.module
        dev = x.device
        x = x.detach().cpu().double()
        with torch.no_grad():
            if net.cfg.MODEL.EXTRA.USE_PRE_NET:
                r, c = net.rgb_preNet, net.cond_preNet
                x0 = self._cbn(r[2], r[3], self._cbn(r[0], r[1], x[:, :3]))
                h = self._cbn(c[0], c[1], x[:, 3:]) + x0
            else:
                h = x[:, :3]
            h = self._out(h, False, self.record["stem"].pop(0) if self.record is not None else None, "stem input")
            h = self._conv(net.conv1, h, relu=True)
            h = self._conv(net.conv2, h, relu=True)
            for m in net.layer1:
                h = self._block(m, h)
            y = [h]
            for s in (2, 3, 4):
                trans = getattr(net, "transition%d" % (s - 1))
                n = getattr(net, "stage%d_cfg" % s)["NUM_BRANCHES"]
                if s == 2:
                    y = [self._trans(trans[i], h) if trans[i] is not None else h for i in range(n)]
                else:
                    y = [self._trans(trans[i], y[-1]) if trans[i] is not None else y[i] for i in range(n)]
                for mod in getattr(net, "stage%d" % s):
                    y = self._module(mod, y)
            return self._conv(net.final_layer, y[0], head=True).float().to(dev)


# regression bound against the fp32 goldens (about 2x the measured 0.153 / 0.142 relative L2 and 0.71 / 0.65
# agreement), NOT the issue's floors: those stay in the strict xfail below
GOLDEN_REGRESSION = {"rel_l2": 0.31, "agree": 0.5}


def _recorded_forward(model, x, monkeypatch):
    """One bf16 forward of `model` with every kernel output kept (see Restated)."""
    from buctd_amd import ops_bf16
    rec = {"conv": {}, "fuse": [], "stem": []}
    conv, fuse, stem = ops_bf16.conv, ops_bf16.fuse_sum, ops_bf16.from_f32

    def conv_(x, wimg, *a, **k):
        y = conv(x, wimg, *a, **k)
        assert wimg.data_ptr() not in rec["conv"], "a convolution ran twice in one forward"
        rec["conv"][wimg.data_ptr()] = y
        return y

    def fuse_(*a, **k):
        rec["fuse"].append(fuse(*a, **k))
        return rec["fuse"][-1]

    def stem_(t):
        rec["stem"].append(stem(t))
        return rec["stem"][-1]
    with monkeypatch.context() as m:
        m.setattr(ops_bf16, "conv", conv_)
        m.setattr(ops_bf16, "fuse_sum", fuse_)
        m.setattr(ops_bf16, "from_f32", stem_)
        with torch.no_grad():
            y = model(x)
    return y, rec


@pytest.mark.parametrize("name", list(NET_BOUNDS))
def test_bf16_network_matches_fp64_restatement(dev, name, monkeypatch):
    """Every step of the wrapper's forward - stem input, each convolution with its bias / residual / ReLU, each fuse row,
    the fp32 head - against the fp64 restatement written from the network's module structure, computed from the same
    bf16 inputs: within the kernel bound of test_bf16_conv_matches_fp64_on_the_same_bf16_operands (fp32 accumulation
    order plus one bf16 rounding).  Every step is visited once, and the heat-maps come out fp32 of the golden shape."""
    from buctd_amd import engine
    gold = np.load(os.path.join(GOLD, f"model_{name}.npz"))
    cfg, net, x = _product(name, dev)
    model = engine.Bf16Inference(net).eval()
    y, rec = _recorded_forward(model, x, monkeypatch)      # CPU input, like the wrapped network accepts
    assert y.dtype == torch.float32 and y.is_cuda and tuple(y.shape) == gold["out"].shape
    n_conv = len(rec["conv"])
    assert n_conv == len(model._net.layers), "not every folded convolution ran exactly once"
    forced = Restated(model, record=rec)
    forced(x.to(dev))
    assert not rec["fuse"] and not rec["stem"], "the wrapper ran fuse rows / stem conversions the network does not have"
    assert len(forced.worst) == n_conv + 1 + sum(len(m.fuse_layers) for s in (2, 3, 4)
                                                 for m in getattr(net, "stage%d" % s) if m.fuse_layers is not None)
    what, ratio = max(forced.worst, key=lambda w: w[1])
    print(f"{name}: {len(forced.worst)} steps, worst error / bound {ratio:.3f} ({what})")
    assert ratio <= 1.0, (what, ratio)
    # free-running: the same computation without teacher forcing (reported; the seeded networks are chaotic)
    free = Restated(model)(x.to(dev))
    f_l2, _, f_agree, _ = heatmap_metrics(y.cpu().numpy(), free.cpu().numpy())
    g_l2, _, g_agree, _ = heatmap_metrics(y.cpu().numpy(), gold["out"])
    print(f"{name}: free-running vs restatement rel L2 {f_l2:.3e} agreement {f_agree:.3f}; vs fp32 golden rel L2 "
          f"{g_l2:.3e} agreement {g_agree:.3f}")
    assert g_l2 <= GOLDEN_REGRESSION["rel_l2"] and g_agree >= GOLDEN_REGRESSION["agree"], (g_l2, g_agree)


# Finding: on these seeded random-weight networks the bf16 error compounds layer by layer (~0.3 % relative
# per convolution, 13-15 % relative L2 at the heat-maps), far outside the floors.  The floors stay as they are; the test
# is a strict xfail so that it turns into a failure the day the mode meets them.
@pytest.mark.xfail(strict=True, raises=AssertionError, reason="bf16 storage does not meet the accuracy floors on the seeded golden networks "
                                       "(measured rel L2 0.153 / 0.142, arg-max agreement 0.71 / 0.65; DESIGN.md 8)")
@pytest.mark.parametrize("name", list(NET_BOUNDS))
def test_bf16_network_against_fp32_goldens(dev, name):
    from buctd_amd import engine
    gold = np.load(os.path.join(GOLD, f"model_{name}.npz"))
    cfg, net, x = _product(name, dev)
    model = engine.Bf16Inference(net).eval()
    with torch.no_grad():
        y = model(x)                               # CPU input, like the wrapped network accepts
    if y.dtype != torch.float32 or tuple(y.shape) != gold["out"].shape:
        raise TypeError(f"bf16 heat-maps {y.dtype} {tuple(y.shape)}")    # not an expected failure
    rel_l2, rel_max, agree, dist = heatmap_metrics(y.cpu().numpy(), gold["out"])
    assert np.array_equal(gold["out"].reshape(*gold["out"].shape[:2], -1).argmax(2), gold["argmax"])
    print(f"{name} bf16: rel L2 {rel_l2:.3e}, max|d|/max|ref| {rel_max:.3e}, argmax agreement {agree:.4f} "
          f"({len(dist)} disagreeing, distances {dist.tolist()})")
    bnd = NET_BOUNDS[name]
    assert rel_l2 <= bnd["rel_l2"] and rel_max <= bnd["rel_max"], (rel_l2, rel_max)
    assert agree >= bnd["agree"], agree
    assert all(d <= 1 for d in dist), dist


def test_fp32_forward_untouched_by_the_bf16_wrapper(dev):
    from buctd_amd import engine
    _, net, x = _product("prenet_w16_96x64", dev)
    with torch.no_grad():
        before = net(x.to(dev))
        model = engine.Bf16Inference(net)
        for _ in range(2):
            model(x)
        after = net(x.to(dev))
    assert torch.equal(before, after)


def _small_cfg():
    from buctd_amd.config import cfg as base, hrnet_extra
    c = base.clone()
    c.defrost()
    c.MODEL.NAME = "pose_hrnet"
    c.MODEL.NUM_JOINTS = 17
    c.MODEL.IMAGE_SIZE = [64, 96]
    c.MODEL.HEATMAP_SIZE = [16, 24]
    c.MODEL.SIGMA = 2
    c.MODEL.PRETRAINED = ""
    c.MODEL.CONDITIONAL_TOPDOWN = True
    c.MODEL.EXTRA = hrnet_extra(16, use_pre_net=True, modules=(1, 2, 2))
    c.DATASET.DATASET = "coco"
    c.DATASET.COLORED = True
    c.TRAIN.LR = 1e-3
    c.freeze()
    return c


def test_bf16_images_follow_every_weight_change(dev):
    """In-place load_state_dict, a FusedAdam step and a train-mode BatchNorm update each make the wrapper's output equal
    a freshly built wrapper's bit for bit."""
    from buctd_amd import engine, models
    from buctd_amd.core.loss import JointsMSELoss
    cfg = _small_cfg()
    torch.manual_seed(21)
    net = models.pose_hrnet.get_pose_net(cfg, is_train=True).to(dev)
    other = models.pose_hrnet.get_pose_net(cfg, is_train=True)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 6, 96, 64, generator=g).to(dev)
    wrap = engine.Bf16Inference(net).eval()

    def check(what):
        with torch.no_grad():
            got = wrap(x)
            fresh = engine.Bf16Inference(net).eval()(x)
        assert torch.equal(got, fresh), what

    with torch.no_grad():
        first = wrap(x)
    # 1. in-place load_state_dict
    net.load_state_dict(other.state_dict())
    check("load_state_dict")
    with torch.no_grad():
        assert not torch.equal(wrap(x), first)
    # 2. one FusedAdam step (and the train-mode BatchNorm updates of its forward)
    model = engine.DataParallel(net)
    opt = engine.get_optimizer(cfg, model)
    model.train()
    t = torch.rand(2, 17, 24, 16, generator=g).to(dev)
    wt = torch.ones(2, 17, 1).to(dev)
    loss = JointsMSELoss(True)(model(x), t, wt)
    opt.zero_grad()
    loss.backward()
    opt.step()
    net.eval()
    check("FusedAdam step")
    # 3. a train-mode forward alone (running statistics written through raw pointers)
    net.train()
    with torch.enable_grad():
        net(x)
    net.eval()
    check("BatchNorm running statistics")


def test_forward_graph_of_the_bf16_wrapper_replays_bit_for_bit(dev):
    from buctd_amd import engine
    _, net, x = _product("prenet_w16_96x64", dev)
    wrap = engine.Bf16Inference(net)
    fg = engine.ForwardGraph(wrap, warmup=1, autoselect=False)
    xd = x.to(dev)
    with torch.no_grad():
        for i in range(4):
            xi = xd + 0.01 * i
            ref = wrap(xi)
            got = fg(xi)
            assert torch.equal(ref, got), i
        assert fg.replays == 3                     # call 0 eager, call 1 captures and replays, calls 2-3 replay
        # a weight change reaches the replayed path too
        with torch.no_grad():
            net.final_layer.bias.add_(0.25)
        assert torch.equal(fg(xd), wrap(xd))


def test_validate_through_the_bf16_wrapper(dev):
    """core.function.validate() with Bf16Inference as `model` (flip test on): its predictions table is within the
    whole-network regression bound of the fp32 validate()."""
    from oracle import recipes
    from buctd_amd import engine, models
    from buctd_amd.core.function import validate
    from buctd_amd.core.loss import JointsMSELoss
    c = _small_cfg().clone()
    c.defrost()
    c.TEST.FLIP_TEST = True
    c.TEST.POST_PROCESS = False
    c.TEST.SHIFT_HEATMAP = True
    c.PRINT_FREQ = 100
    c.freeze()
    _, omodel, x, _ = recipes.build("prenet_w16_96x64")
    net = models.pose_hrnet.get_pose_net(c, is_train=False)
    net.load_state_dict(omodel.state_dict(), strict=True)
    net = net.to(dev).eval()

    class Dataset:
        flip_pairs = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]
        image_size = c.MODEL.IMAGE_SIZE
        kpt_colors = [[(37 * k) % 256, (91 * k) % 256, (53 * k) % 256] for k in range(17)]

        def __init__(self, n):
            self.n, self.captured = n, None

        def __len__(self):
            return self.n

        def evaluate(self, cfg, preds, output_dir, all_boxes, img_path, *a, **k):
            self.captured = preds.copy()
            return {"AP": 0.0}, 0.0

    n = x.shape[0]
    batches = []
    for i in range(2):
        g = torch.Generator().manual_seed(960 + i)
        xi = x + 0.02 * i * torch.randn(x.shape, generator=g)
        meta = {"center": torch.rand(n, 2, generator=g) * 100 + 50, "scale": torch.ones(n, 2) * 0.5,
                "score": torch.rand(n, generator=g), "annotation_id": torch.arange(n) + n * i,
                "image": [f"im_{i}_{j}.jpg" for j in range(n)],
                "cond_joints": torch.cat([torch.rand(n, 17, 2, generator=g) * 60, torch.zeros(n, 17, 1)], 2),
                "cond_joints_vis": torch.ones(n, 17, 3)}
        batches.append((xi, torch.zeros(n, 17, 24, 16), torch.ones(n, 17, 1), meta))
    wrap = engine.Bf16Inference(net)
    calls = []
    wrap.register_forward_hook(lambda *a: calls.append(1))
    tables = []
    for model in (net, wrap):
        ds = Dataset(2 * n)
        validate(c, batches, ds, model, JointsMSELoss(True), "/tmp", "/tmp", None)
        tables.append(ds.captured)
    assert len(calls) >= 2, "validate() did not run through the wrapper"
    fp32, bf = tables
    assert bf.shape == fp32.shape and np.isfinite(bf).all()
    # the whole-network regression bound (GOLDEN_REGRESSION) on the decoded predictions: the share of key points whose
    # prediction equals the fp32 validate()'s
    px = 0.5 * 200 / 16
    d = np.abs(bf[:, :, :2] - fp32[:, :, :2]).max(axis=2)
    same = float((d < 1e-3 * px).mean())
    print(f"validate bf16 vs fp32: identical {same:.3f}, max shift {float(d.max() / px):.2f} px")
    assert same >= GOLDEN_REGRESSION["agree"], same
