"""The general calling form of the fused attention (attn_mha.hip / attn_mha_train.hip): h heads, q / k / v as separate
tensors with their own row strides, token counts that end in a masked half block (T % 64 == 0).  Nothing T x T in memory.
Bar: the project's bar for attention, 2e-5 relative L2 against the fp64 formula of test_position_attention
(reference lib/models/self_attention.py:74-87), evaluated here in fp64 by torch on the device."""
import copy
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

BAR = 2e-5
HEADS = (1, 2, 3, 6, 7)
WIDTHS = (16, 32, 48, 96, 128)


def _e(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def _ref64(q, k, v, h, dout=None):
    """softmax(q k^T / sqrt(dh)) v per head in fp64 (+ dq, dk, dv for dout)"""
    q, k, v = (t.detach().double().requires_grad_(dout is not None) for t in (q, k, v))
    B, T, hd = q.shape
    dh = hd // h
    qh = q.view(B, T, h, dh).permute(0, 2, 1, 3)
    kh = k.view(B, T, h, dh).permute(0, 2, 3, 1)
    vh = v.view(B, T, h, dh).permute(0, 2, 1, 3)
    att = torch.softmax(torch.matmul(qh, kh) / math.sqrt(dh), -1)
    out = torch.matmul(att, vh).permute(0, 2, 1, 3).contiguous().view(B, T, hd)
    if dout is None:
        return out.detach()
    out.backward(dout.double())
    return out.detach(), q.grad, k.grad, v.grad


def _operands(B, T, h, dh, layout, dev, seed):
    """-> q, k, v leaves' views: 'packed' = q | k halves of one tensor (k is None), 'views' = channel slices of wider
    tensors (row strides larger than h * dh)"""
    g = torch.Generator().manual_seed(seed)
    hd = h * dh
    if layout == "packed":
        qk = (torch.randn(B, T, 2 * hd, generator=g) * 1.2)
        qk[:, ::7, :hd] *= 3.0                  # a few peaked rows: the online rescaling works
        v = torch.randn(B, T, hd, generator=g)
        return qk.to(dev), None, v.to(dev)
    big = torch.randn(3, B, T, hd + 16, generator=g) * 1.2
    big[0, :, ::7] *= 3.0
    big = big.to(dev)
    return big[0, :, :, 8:8 + hd], big[1, :, :, 4:4 + hd], big[2, :, :, 12:12 + hd]


@pytest.mark.parametrize("T,d,h", [(3072, 112, 7), (3072, 96, 2), (3072, 96, 6), (1728, 96, 2), (6912, 96, 2), (192, 96, 6),
                                   (3072, 112, 1), (1728, 48, 1)])
def test_dispatch_takes_heads_and_half_blocks(dev, T, d, h):
    from buctd_amd import ops
    assert ops.mha_fused_ok(T, d, h) and ops.mha_train_ok(T, d, h)
    lib = ops.lib()
    assert lib.buctd_mha_heads_fwd_supported(T, h, d // h) == 1 and lib.buctd_mha_heads_train_supported(T, h, d // h) == 1
    assert lib.buctd_mha_heads_bwd_workspace(3, h, T) == 3 * h * T * 4


def test_dispatch_leaves_the_rest_on_the_materialised_path(dev):
    from buctd_amd import ops
    for T, d, h in [(432, 96, 2), (100, 96, 2), (3072, 112, 2), (3072, 112, 4), (3072, 192, 1), (3072, 96, 5), (3072, 40, 2)]:
        assert not ops.mha_fused_ok(T, d, h) and not ops.mha_train_ok(T, d, h), (T, d, h)


@pytest.mark.parametrize("layout", ["packed", "views"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T", [128, 192, 320, 1728])
def test_general_form_vs_fp64(dev, T, B, layout):
    """eval forward in both math modes, training forward with p = 0 and dq, dk, dv for every (h, dh)"""
    from buctd_amd import ops
    bad = []
    for h in HEADS:
        for dh in WIDTHS:
            hd = h * dh
            q, k, v = _operands(B, T, h, dh, layout, dev, T * 31 + B * 7 + h * 131 + dh)
            q64, k64 = (q[..., :hd], q[..., hd:]) if k is None else (q, k)
            dout = torch.randn(B, T, hd, generator=torch.Generator().manual_seed(h + dh)).to(dev)
            ref, rq, rk, rv = _ref64(q64, k64, v, h, dout)
            old = ops.get_conv_math()
            for mode in ("fp32", "bf16x6"):
                ops.set_conv_math(mode)
                try:
                    out = ops.mha_fwd(q, v, h=h, k=k)
                finally:
                    ops.set_conv_math(old)
                bad += [(f"eval[{mode}]", h, dh, _e(out, ref))]
            ql = q.detach().clone().requires_grad_(True) if k is None else None
            if k is None:
                vl = v.detach().clone().requires_grad_(True)
                out = ops.FusedMHA.apply(ql, vl, 0.0, True, h)
                out.backward(dout)
                got = (ql.grad[..., :hd], ql.grad[..., hd:], vl.grad)
            else:
                bases = [t.detach().clone().requires_grad_(True) for t in (q._base, k._base, v._base)]
                off = (8, 4, 12)
                qv, kv, vv = (b[i, :, :, off[i]:off[i] + hd] for i, b in enumerate(bases))
                out = ops.FusedMHA.apply(qv, vv, 0.0, True, h, kv)
                out.backward(dout)
                got = tuple(b.grad[i, :, :, off[i]:off[i] + hd] for i, b in enumerate(bases))
                for i, b in enumerate(bases):            # nothing lands outside the slices
                    rest = b.grad.clone()
                    rest[i, :, :, off[i]:off[i] + hd] = 0
                    assert not rest.any()
            bad += [("train out", h, dh, _e(out.detach(), ref)), ("dq", h, dh, _e(got[0], rq)), ("dk", h, dh, _e(got[1], rk)),
                    ("dv", h, dh, _e(got[2], rv))]
    worst = max(bad, key=lambda r: r[3])
    print(f"T{T} B{B} {layout}: worst {worst[0]} h{worst[1]} dh{worst[2]} rel err {worst[3]:.2e} over {len(bad)} figures")
    over = [r for r in bad if not r[3] <= BAR]
    assert not over, f"T{T} B{B} {layout}: over {BAR}: {over[:8]}"


def test_nothing_t_by_t_is_allocated(dev):
    from buctd_amd import ops
    B, T, h, dh = 2, 3072, 2, 48
    q, k, v = _operands(B, T, h, dh, "views", dev, 5)
    q, k, v = (t.contiguous().requires_grad_(True) for t in (q, k, v))
    dout = torch.randn(B, T, h * dh, device=dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = ops.FusedMHA.apply(q, v, 0.1, True, h, k)
    out.backward(dout)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"peak {peak} bytes, bound {4 * B * T * T // 2}")
    assert peak < 4 * B * T * T // 2, "the fused path must not allocate anything T x T"


def _drop_run(ops, fused, q, k, v, h, dout, p=0.3):
    ql, kl, vl = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    if fused:
        out = ops.FusedMHA.apply(ql, vl, p, True, h, kl)
    else:
        out = ops.PositionAttention.apply(ql, kl, vl, h, p, True)
    out.backward(dout)
    return out.detach(), ql.grad, kl.grad, vl.grad


@pytest.mark.parametrize("device_seed", [False, True])
@pytest.mark.parametrize("T,h,dh", [(256, 2, 48), (192, 7, 16), (320, 2, 32)])
def test_same_masks_as_the_materialised_path(dev, T, h, dh, device_seed):
    """the counter of element (b, head, row, col) is the one of the materialised [B, h, T, T] tensor: fused and
    PositionAttention agree seed for seed - as launch argument and read from a device seed table"""
    from buctd_amd import ops
    B = 3
    g = torch.Generator().manual_seed(T + h)
    q, k, v, dout = (torch.randn(B, T, h * dh, generator=g).to(dev) for _ in range(4))
    table = torch.zeros(4, dtype=torch.int64, device=dev)
    seeds = (0x1234567890ABCDEF, 0x0FEDCBA987654321)
    table[0], table[1] = seeds[0], seeds[1]

    def run(fused, which):
        if device_seed:
            s = ops.DeviceSeed(table, which)
        else:
            s = seeds[which]
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(ops, "next_seed", lambda: s)
            return _drop_run(ops, fused, q, k, v, h, dout)

    fused, mat, other = run(True, 0), run(False, 0), run(False, 1)
    nodrop = ops.FusedMHA.apply(q, v, 0.3, False, h, k)
    assert (fused[0] - nodrop).abs().max().item() > 1e-2, "dropout must change the output"
    for name, a, b, c in zip(("out", "dq", "dk", "dv"), fused, mat, other):
        err, ctl = _e(a, b), _e(a, c)
        print(f"T{T} h{h} dh{dh} dseed={device_seed} {name}: same seed {err:.2e}, other seed {ctl:.2e}")
        assert err <= BAR, f"fused vs materialised with dropout: {name} rel err {err:.2e}"
        assert ctl > BAR, f"control: another seed must be visible in {name} ({ctl:.2e})"


def _args(ops, B, T, h, dh, q, k, v, ldq, ldk, ldv, out, lse, p=0.0):
    from buctd_amd import _C
    a = _C.MhaArgs()
    a.B, a.T, a.h, a.dh = B, T, h, dh
    a.q, a.k, a.v, a.ldq, a.ldk, a.ldv = q, k, v, ldq, ldk, ldv
    a.out, a.ldo, a.lse = out.data_ptr(), h * dh, (lse.data_ptr() if lse is not None else None)
    a.scale, a.p_drop = 1.0 / math.sqrt(dh), p
    return a


@pytest.mark.parametrize("B,T,d", [(2, 384, 48), (1, 3072, 112), (3, 128, 16), (2, 256, 128), (2, 256, 96)])
def test_host_ops_reach_the_general_entry_points(dev, B, T, d, monkeypatch):
    """packed one-head ops.FusedMHA (dropout on) and ops.mha_fwd (in-kernel split, both math modes) are the general entry
    points with h = 1, k = q + d: out, d(q | k), dv identical bit for bit"""
    from buctd_amd import ops
    lib, sp = ops.lib(), ops.stream_ptr
    g = torch.Generator().manual_seed(B * T + d)
    qk = (torch.randn(B, T, 2 * d, generator=g) * 1.5).to(dev)
    v = torch.randn(B, T, d, generator=g).to(dev)
    dout = torch.randn(B, T, d, generator=g).to(dev)
    qp, kp, vp = qk.data_ptr(), qk.data_ptr() + 4 * d, v.data_ptr()
    p, seed = 0.2, 0xABCDEF12345
    new = lambda *s: torch.empty(*s, device=dev)
    o1, l1 = new(B, T, d), new(B, 1, T)
    a = _args(ops, B, T, 1, d, qp, kp, vp, 2 * d, 2 * d, d, o1, l1, p)
    ops.check(lib.buctd_mha_heads_fwd_train(ctypes.byref(a), seed, sp()), "general")
    g1, dv1 = new(B, T, 2 * d), new(B, T, d)
    ws = ops.workspace(lib.buctd_mha_heads_bwd_workspace(B, 1, T), qk.device)
    a.dout, a.lddo = dout.data_ptr(), d
    a.dq, a.dk, a.dv, a.lddq, a.lddk, a.lddv = g1.data_ptr(), g1.data_ptr() + 4 * d, dv1.data_ptr(), 2 * d, 2 * d, d
    ops.check(lib.buctd_mha_heads_bwd(ctypes.byref(a), seed, ws.data_ptr(), ws.numel(), sp()), "general")
    ql, vl = qk.clone().requires_grad_(True), v.clone().requires_grad_(True)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops, "next_seed", lambda: seed)
        out = ops.FusedMHA.apply(ql, vl, p, True)
        out.backward(dout)
    assert torch.equal(out.detach(), o1) and torch.equal(ql.grad, g1) and torch.equal(vl.grad, dv1)
    # eval
    monkeypatch.setattr(ops, "_MHA_PRESPLIT", False)
    old = ops.get_conv_math()
    for mode, gen_fn in (("bf16x6", lib.buctd_mha_heads_fwd_bf16x6), ("fp32", lib.buctd_mha_heads_fwd)):
        o2 = new(B, T, d)
        ops.check(gen_fn(ctypes.byref(_args(ops, B, T, 1, d, qp, kp, vp, 2 * d, 2 * d, d, o2, None)), sp()), "general")
        ops.set_conv_math(mode)
        try:
            out = ops.mha_fwd(qk, v)
        finally:
            ops.set_conv_math(old)
        assert torch.equal(out, o2), mode


@pytest.mark.parametrize("T,h,layout,presplit", [(128, 1, "packed", True), (192, 1, "packed", False), (128, 1, "views", False),
                                                 (128, 2, "packed", False)])
def test_only_the_packed_one_head_form_takes_the_presplit_kernel(dev, T, h, layout, presplit, monkeypatch):
    """which C entry ops.mha_fwd calls in the default (bf16x6) mode: the pre-split kernel for the packed one-head form in
    whole 128-query tiles, the in-kernel split for everything else - the smallest shape on each side of every condition"""
    from buctd_amd import ops
    lib = ops.lib()
    calls = {}
    for name in ("buctd_mha_heads_fwd_bf16x6_ws", "buctd_mha_heads_fwd_bf16x6", "buctd_mha_heads_fwd"):
        def wrapped(*a, _n=name, _fn=getattr(lib, name)):
            calls[_n] = calls.get(_n, 0) + 1
            return _fn(*a)
        monkeypatch.setattr(lib, name, wrapped)
    assert ops.get_conv_math() == "bf16x6" and ops._MHA_X6 and ops._MHA_PRESPLIT
    B, dh = 2, 16
    q, k, v = _operands(B, T, h, dh, layout, dev, T + h)
    out = ops.mha_fwd(q, v, h=h, k=k)
    assert calls == {"buctd_mha_heads_fwd_bf16x6_ws" if presplit else "buctd_mha_heads_fwd_bf16x6": 1}, calls
    q64, k64 = (q[..., :h * dh], q[..., h * dh:]) if k is None else (q, k)
    err = _e(out, _ref64(q64, k64, v, h))
    assert err <= BAR, err


# ---------------------------------------------------------------------------------------------------------- models ----
def _spy(monkeypatch, ops):
    calls = {"fused": 0, "materialised": 0}
    raw_f, raw_e, raw_m = ops.FusedMHA.apply, ops.mha_fwd, ops.PositionAttention.apply

    def count(key, fn):
        def wrapped(*a, **kw):
            calls[key] += 1
            return fn(*a, **kw)
        return wrapped

    monkeypatch.setattr(ops.FusedMHA, "apply", count("fused", raw_f))
    monkeypatch.setattr(ops, "mha_fwd", count("fused", raw_e))
    monkeypatch.setattr(ops.PositionAttention, "apply", count("materialised", raw_m))
    return calls


def _set_dropout(net, p):
    from buctd_amd.models.transpose_h import MultiheadAttention
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = p
        if isinstance(m, MultiheadAttention):
            m.dropout = p


def _model_pair(net, x, fused_off, calls):
    """eval forward and one train-mode forward + backward (dropout 0), fused dispatch on and off -> two result lists"""
    res = []
    state = copy.deepcopy(net.state_dict())      # the train-mode forward moves the BatchNorm running statistics
    for off in (False, True):
        with fused_off(off):
            net.load_state_dict(state)
            before = dict(calls)
            net.eval()
            with torch.no_grad():
                y_eval = net(x)
            net.train()
            for p in net.parameters():
                p.grad = None
            y = net(x)
            y = y[-1] if isinstance(y, list) else y
            (y * torch.linspace(0.5, 1.5, y.numel(), device=y.device).view(y.shape)).sum().backward()
            took = {k: calls[k] - before[k] for k in calls}
            res.append(([y_eval.detach().clone(), y.detach().clone()],
                        {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}, took))
    (outs_f, grads_f, took_f), (outs_m, grads_m, took_m) = res
    assert took_f["fused"] >= 2 and took_m["fused"] == 0 and took_m["materialised"] > took_f["materialised"], (took_f, took_m)
    for a, b in zip(outs_f, outs_m):
        assert _e(a, b) <= BAR, _e(a, b)
    assert grads_f.keys() == grads_m.keys() and len(grads_f) > 10

    def err(n):
        # fc_k.bias: a constant added to every key shifts all logits of a row alike, the soft-max does not see it - this
        # gradient (the sum of dk over the tokens) is zero in exact arithmetic and pure round-off in fp32 on either path.
        # It is measured against its twin of the same shape and scale, the sum of dq over the tokens (fc_q.bias).
        if n.endswith("fc_k.bias"):
            scale = grads_m[n[:-len("fc_k.bias")] + "fc_q.bias"].double().norm()
            return ((grads_f[n].double() - grads_m[n].double()).norm() / scale).item()
        return _e(grads_f[n], grads_m[n])

    worst = max((err(n), n) for n in grads_f if grads_m[n].abs().max() > 0)
    print("model: outputs", [f"{_e(a, b):.2e}" for a, b in zip(outs_f, outs_m)], "worst gradient", worst, took_f, took_m)
    assert worst[0] <= BAR, worst


class _MhaOff:
    """monkeypatched mha_*_ok: every shape on the materialised path"""

    def __init__(self, ops):
        self.ops = ops

    def __call__(self, off):
        mp = pytest.MonkeyPatch()
        if off:
            mp.setattr(self.ops, "mha_fused_ok", lambda *a, **k: False)
            mp.setattr(self.ops, "mha_train_ok", lambda *a, **k: False)
        return _Ctx(mp)


class _Ctx:
    def __init__(self, mp):
        self.mp = mp

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.mp.undo()


@pytest.mark.parametrize("heads,cond", [(2, False), (6, False), (7, True)])
def test_transpose_h_with_heads_takes_the_fused_kernels(dev, heads, cond, monkeypatch):
    from oracle import cfg as ocfg
    from buctd_amd import models, ops
    c = ocfg.hrnet_cfg(16, 17, (48, 64), "transpose_h", use_attention=cond, stage_modules=(1, 1, 1))
    c.MODEL.DIM_MODEL = 96            # + 16 condition channels = 112 with the condition: 7 heads of 16
    c.MODEL.DIM_FEEDFORWARD = 64
    c.MODEL.ENCODER_LAYERS = 2
    c.MODEL.N_HEAD = heads
    torch.manual_seed(3)
    net = models.transpose_h.get_pose_net(c, is_train=True).to(dev)
    _set_dropout(net, 0.0)
    c1 = copy.deepcopy(c)
    c1.MODEL.N_HEAD = 1
    assert models.transpose_h.get_pose_net(c1, is_train=True).state_dict().keys() == net.state_dict().keys()
    x = torch.randn(2, 6 if cond else 3, 64, 48, generator=torch.Generator().manual_seed(1)).to(dev)
    _model_pair(net, x, _MhaOff(ops), _spy(monkeypatch, ops))


def _coam_cfg(heads=1, att=(False, True, False, False), selfatt=(False, False, False, False), width=16):
    from buctd_amd.config import cfg as base, hrnet_extra
    c = base.clone()
    c.defrost()
    c.MODEL.NAME = "pose_hrnet_coam"
    c.MODEL.NUM_JOINTS = 14
    c.MODEL.IMAGE_SIZE = [32, 96]             # 8 x 24 = 192 tokens on the first branch, 48 and 12 below
    c.MODEL.HEATMAP_SIZE = [8, 24]
    c.MODEL.ATT_MODULES = list(att)
    c.MODEL.SELFATT_MODULES = list(selfatt)
    c.MODEL.ATTENTION_HEADS = heads
    c.MODEL.CONDITIONAL_TOPDOWN = True
    c.MODEL.EXTRA = hrnet_extra(width, use_attention=True, modules=(1, 1, 1))
    c.DATASET.COLORED = True
    c.freeze()
    return c


class _FusedFlagOff:
    """ScaledDotProductAttention.fused = False: the comparison side"""

    def __init__(self, net):
        from buctd_amd.models.self_attention import ScaledDotProductAttention
        self.mods = [m for m in net.modules() if isinstance(m, ScaledDotProductAttention)]
        assert self.mods

    def __call__(self, off):
        for m in self.mods:
            m.fused = not off
        return _Ctx(pytest.MonkeyPatch())


def test_coam_with_two_heads_takes_the_fused_kernels(dev, monkeypatch):
    from buctd_amd import models, ops
    torch.manual_seed(5)
    net = models.pose_hrnet_coam.get_pose_net(_coam_cfg(heads=2), is_train=True).to(dev)
    _set_dropout(net, 0.0)
    x = torch.randn(2, 6, 96, 32, generator=torch.Generator().manual_seed(2)).to(dev)
    try:
        _model_pair(net, x, _FusedFlagOff(net), _spy(monkeypatch, ops))
    finally:
        _FusedFlagOff(net)(False)


def test_self_attention_module_takes_the_fused_kernels(dev, monkeypatch):
    """MODEL.SELFATT_MODULES builds SelfAttentionModule (q, k, v = three projections of the feature map); the network's
    forward only enters the ATT_MODULES blocks, so the module built by the option is driven directly.  Width 32: with 16
    channels the narrow-contraction kernel (at most 19 + 1) takes the first branch, as it did before"""
    from buctd_amd import models, ops
    from buctd_amd.models.pose_hrnet_coam import SelfAttentionModule
    torch.manual_seed(6)
    net = models.pose_hrnet_coam.get_pose_net(_coam_cfg(att=(False,) * 4, selfatt=(False, True, False, False), width=32), is_train=True)
    mod = net.stage2_att.to(dev)
    assert isinstance(mod, SelfAttentionModule)
    _set_dropout(mod, 0.0)
    for p in mod.parameters():               # the constructor's std = 0.001 would leave the logits flat
        torch.nn.init.normal_(p, std=0.15)
    g = torch.Generator().manual_seed(3)
    xs = [torch.randn(2, 24, 8, 32, generator=g).to(dev), torch.randn(2, 12, 4, 64, generator=g).to(dev),
          torch.randn(2, 6, 2, 128, generator=g).to(dev)]

    class Wrap(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.mod = mod

        def forward(self, x):
            ys = self.mod(xs)
            return ys[0].reshape(2, -1) + 0 * x.sum()

    calls = _spy(monkeypatch, ops)
    try:
        _model_pair(Wrap(), torch.zeros(1, device=dev), _FusedFlagOff(mod), calls)
    finally:
        _FusedFlagOff(mod)(False)


def test_step_graph_with_heads_and_fresh_masks_equals_eager(dev, monkeypatch):
    """the two-head CoAM network with dropout on under StepGraph(fresh_dropout_masks=True): three steps bit-identical to
    the eager loop (the _dseed forms of the general entry points)"""
    from buctd_amd import engine, models, ops
    from buctd_amd.core.loss import JointsMSELoss
    cfg = _coam_cfg(heads=2)
    torch.manual_seed(11)
    net = models.pose_hrnet_coam.get_pose_net(cfg, is_train=True).to(dev)
    pairs = []
    for i in range(2):
        model = engine.DataParallel(net if i == 0 else copy.deepcopy(net))
        opt = engine.get_optimizer(cfg, model)
        model.train()
        pairs.append((model, opt))
    (eager, eopt), (graphed, gopt) = pairs
    crit = JointsMSELoss(True)
    calls = _spy(monkeypatch, ops)

    def batch(seed):
        g = torch.Generator().manual_seed(seed)
        return (torch.randn(2, 6, 96, 32, generator=g).to(dev), torch.rand(2, 14, 24, 8, generator=g).to(dev),
                (torch.rand(2, 14, 1, generator=g) < 0.8).float().to(dev))

    batches = [batch(900 + i) for i in range(5)]          # two warm-up steps, then three captured / replayed ones
    ops.manual_seed(0x5EED)
    ref = []
    for x, t, w in batches:
        ops.set_grad_arena(eopt.flat)
        loss = crit(eager(x), t, w)
        eopt.zero_grad()
        loss.backward()
        eopt.step()
        ref.append(loss.detach().clone())
    assert calls["fused"] >= 5
    ops.manual_seed(0x5EED)
    ops.set_grad_arena(gopt.flat)
    step = engine.StepGraph(graphed, crit, gopt, warmup=2, streams="single", fresh_dropout_masks=True)
    for i, b in enumerate(batches):
        ops.set_grad_arena(gopt.flat)
        _, loss = step(*b)
        assert torch.equal(loss.detach(), ref[i]), (i, float(loss), float(ref[i]))
    assert step.replays == 3
    assert torch.equal(eopt.flat.flat, gopt.flat.flat)
