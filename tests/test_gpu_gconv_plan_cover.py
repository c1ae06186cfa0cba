"""Every case of tests/helpers/gconv_cases.py x every option set of the gathered bf16x6 convolutions (conv_gather_x6.hip: the
tiled gconv_x6_kernel and the row-streaming conv1x1_rows_x6_kernel; conv_gather_wgrad.hip) against an fp64 CPU evaluation of the
SAME operation (torch conv2d / conv_transpose2d / conv2d_weight in double on the float inputs), per element.  The host-only
closure test (test_gconv_plan_cover.py) proves that the cases reach every route, tile plan, epilogue and weight-gradient plan.

Metrics and bars (those of test_gpu_conv3x3_plan_cover.py; none of them taken from what the kernels give):
  convolution outputs   |err| / (sum of the absolute values of the terms of the element: conv(|x|, |w|) + |bias| + |residual|)
                        <= 2e-6 and <= 3 x (the same ratio of the exact-fp32 kernel on the same inputs) + 2e-7;
  forward statistics    the bars of test_gpu_bn_acc.py (mean 2e-6 max(1, max |mu|), invstd 3e-7, running_var 1e-6 relative, applied
                        output 2e-5 max(1, |y|)) against fp64 statistics of the device's own z;
  weight gradient       |err| / conv2d_weight(|x|, |dy|) under the same two bars; run-to-run bit-equal; accumulate = 1.
Each convolution bar is asserted on the whole tensor, on the last position tile, the last column tile (BM / BN of the plan
query; 32 rows / 64 columns - a row block and a staging slice - for the row kernel), the border pixels and, for a stride-2
data gradient, on each of the four parity classes; the message names the worst element (n, h, w, c).  The ratios themselves
are formed in fp64 on the device from the CPU's fp64 reference (the largest case writes 35 M elements).

Measured on an MI355X: worst figure per (route, option set) over all cases next to the baseline it was judged against (the
exact-fp32 kernel's ratio on the same inputs for the convolution outputs, the 3e-7 bar for invstd).  The worst tiled ratios all
come from the stride-2 hard-operands case; the row kernel has random-normal cases only:
  route, option set        conv ratio / fp32 kernel   invstd (bar 3e-7)
  tiled general            5.63e-07 / 5.67e-07
  tiled general-affine     5.25e-07 / 4.07e-07
  tiled plain              5.45e-07 / 5.61e-07
  tiled STATS              5.45e-07 / 5.61e-07        1.2e-07
  tiled partials           5.45e-07 / 5.61e-07        8.9e-08
  tiled fwd-RES            5.35e-07 / 5.73e-07
  tiled RES (dgrad)        4.99e-07 / 6.05e-07
  rows plain               3.39e-07 / 3.61e-07
  rows bias                3.04e-07 / 3.85e-07
  rows RES                 3.32e-07 / 3.25e-07
  rows STATS               3.39e-07 / 3.61e-07        5.8e-08
  rows STATS+bias          3.04e-07 / 3.85e-07        5.9e-08
  wgrad                    2.87e-07 / 4.16e-07
Wall time of the module: 11-13 s (197 tests, the slowest 0.8 s after the first one's start-up).  No case exposed a fault of
the kernels: the pad half-step of the prepared image is written (as zeros) by buctd_gconv_x6_prep, and every guard-band run is
bit-equal to the plain one.

The mean of the statistics is held to the bar exactly as test_gpu_bn_acc.py states it - the largest deviation against
2e-6 max(1, max |mean| of the tensor).  Per channel (the 3x3 module's reading) the stride-2 hard-operands case measures
2.9e-06 max(1, |mean|) on a channel with sigma 747 at |mean| 1.4 over 30 rows, where one fp32 ulp of a single z is 3e-5."""
import ctypes as C
import math
import time

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import gconv_cases as T
# the operand generator, the BatchNorm stand-in and the guard-band mechanics of the 3x3 module (shared, not copied)
from tests.helpers.guard_bands import SENTINEL, banded, untouched
from tests.test_gpu_conv3x3_plan_cover import _Bn, hard_operands, in_fp32, x6  # noqa: F401

pytestmark = pytest.mark.gpu

WORST = {}
T0 = time.time()


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nworst figures per (route, option set) (measured / baseline, case):")
    for k in sorted(WORST):
        v = WORST[k]
        print(f"  {k:36s} {v[0]:.3e} / {v[1]:.3e}  at {v[2]}")
    print(f"wall time of the module: {time.time() - T0:.1f} s")


def _note(key, val, base, where):
    if key not in WORST or val > WORST[key][0]:
        WORST[key] = (val, base, where)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def wcl(w):
    return w.contiguous(memory_format=torch.channels_last)


def geo(kind):
    """(filter size, stride, pad)"""
    return (1, 1, 0) if kind == 1 else (3, 2, 1)


class Inputs:
    """the float operands of one case (on the CPU; NHWC copies on the device) and the fp64 reference built from them"""

    def __init__(self, case, hard, dev):
        kind, d, N, H, W, Ci, Co = case
        k, st, pad = geo(kind)
        self.case, self.hard, self.dev = case, hard, dev
        g = torch.Generator().manual_seed(sum(case) * 31 + Ci)
        ishape, oshape = T.in_shape(case), T.out_shape(case)
        nchw_of = lambda s: (s[0], s[3], s[1], s[2])
        if hard:
            # exponents 2^-20..2^20 inside one reduction, moved down so that the sums of squares of the outputs stay inside the
            # range of the statistics accumulator (bn_acc.h) - the operands of the 3x3 module's hard case
            src = hard_operands(nchw_of(ishape), g, -20, 20, -14)
            w = hard_operands((Co, Ci, k, k), g, -8, 8, -6)
            res = hard_operands(nchw_of(oshape), g, -20, 20, -14)
        else:
            src = torch.randn(nchw_of(ishape), generator=g) + 0.5
            w = torch.randn(Co, Ci, k, k, generator=g) / math.sqrt(k * k * ishape[3])
            res = torch.randn(nchw_of(oshape), generator=g)
        nout = oshape[3]
        self.bias = torch.randn(nout, generator=g)
        self.scale, self.shift = torch.rand(nout, generator=g) + 0.5, torch.randn(nout, generator=g)
        s64, w64 = src.double(), w.double()
        if d == T.FWD:
            f = lambda a, b: F.conv2d(a, b, None, st, pad)
        else:
            f = lambda a, b: F.conv_transpose2d(a, b, None, st, pad, output_padding=st - 1)
        # fp64 on the CPU: the value and the sum of the absolute values of its terms; kept on the device as doubles
        self.ref = nhwc(f(s64, w64)).to(dev)
        self.mag = nhwc(f(s64.abs(), w64.abs())).to(dev)
        assert tuple(self.ref.shape) == oshape
        self.src, self.w, self.res = nhwc(src).to(dev), wcl(w).to(dev), nhwc(res).to(dev)
        self.x_shape = (N, H, W, Ci)
        self.memo = {}

    def get(self, key, fn):
        if key not in self.memo:
            self.memo[key] = fn()
        return self.memo[key]


_last = {}


def inputs(case, hard, dev):
    if _last.get("key") != (case, hard):
        _last.clear()
        _last.update(key=(case, hard), inp=Inputs(case, hard, dev))
    return _last["inp"]


def regions(case, pl, dev):
    """{name: (pixel mask [N, H, W, 1] or None, channel mask [C] or None)} over the tensor the launch writes"""
    kind, d, N, H, W, Ci, Co = case
    oN, oH, oW, oC = T.out_shape(case)
    n, y, x = torch.meshgrid(torch.arange(oN, device=dev), torch.arange(oH, device=dev), torch.arange(oW, device=dev), indexing="ij")
    par = kind == 2 and d == T.DGRAD
    out = {"whole tensor": (None, None)}
    if pl["route"] == 1:
        row = (n * oH + y) * oW + x
        out["last row block"] = ((row // 32 == (oN * oH * oW - 1) // 32)[..., None], None)
        out["last 64 columns"] = (None, torch.arange(oC, device=dev) >= oC - 64)
    else:
        gy, gx = (y // 2, x // 2) if par else (y, x)
        Hg, Wg = (oH // 2, oW // 2) if par else (oH, oW)
        p = n * (Hg + 1) * (Wg + 2) + (gy + 1) * (Wg + 2) + gx + 1        # the padded flattened position of a grid pixel
        out["last position tile"] = ((p // pl["BM"] == int(p.max()) // pl["BM"])[..., None], None)
        out["last column tile"] = (None, torch.arange(oC, device=dev) >= oC - pl["BN"])
    out["border pixels"] = (((y == 0) | (y == oH - 1) | (x == 0) | (x == oW - 1))[..., None], None)
    if par:
        for a in (0, 1):
            for b in (0, 1):
                out[f"parity class ({a}, {b})"] = (((y % 2 == a) & (x % 2 == b))[..., None], None)
    return out


def check_conv(name, opt, case, hard, pl, got, got32, ref, mag):
    """got / got32: the bf16x6 and the exact-fp32 kernel's output (NHWC, device); ref / mag: fp64 value and sum of |terms|"""
    cid = T.case_id(case) + ("-hard" if hard else "")
    route = "rows" if pl["route"] else "tiled"
    mag = mag.clamp_min(1e-300)
    r = (got.double() - ref).abs() / mag
    r32 = float(((got32.double() - ref).abs() / mag).max())
    bar = min(2e-6, 3 * r32 + 2e-7)
    worst = float(r.max())
    at = tuple(int(v) for v in torch.unravel_index(r.argmax(), r.shape))
    print(f"{route} {opt} {name} {cid}: error / sum|terms| bf16x6 {worst:.3e}, exact-fp32 kernel {r32:.3e} (bar {bar:.3e}); plan {pl}")
    _note(f"{route} {opt}: conv", worst, r32, cid)
    assert torch.isfinite(got).all(), f"{opt} {name} {cid}: non-finite output"
    zero = torch.zeros((), dtype=r.dtype, device=r.device)
    for where, (pm, cm) in regions(case, pl, r.device).items():
        rr = r
        if pm is not None:
            rr = torch.where(pm, rr, zero)
        if cm is not None:
            rr = torch.where(cm, rr, zero)
        w_ = float(rr.max())
        a_ = tuple(int(v) for v in torch.unravel_index(rr.argmax(), rr.shape))
        assert w_ <= bar, (f"{route} {opt} {name} {cid} [{where}]: error / sum|terms| {w_:.3e} > {bar:.3e} at (n, h, w, c) = {a_} "
                           f"(fp32 kernel {r32:.3e}; worst of the tensor {worst:.3e} at {at}; plan {pl})")


def check_stats(name, opt, case, hard, pl, z, mean, invstd, bn, y=None, res=None):
    """forward statistics against fp64 statistics of the device's own z (on the CPU)"""
    cid = T.case_id(case) + ("-hard" if hard else "")
    Cn = z.shape[-1]
    zd = z.double().cpu().reshape(-1, Cn)
    rows = zd.shape[0]
    mu, var = zd.mean(0), zd.var(0, unbiased=False)
    ist = 1.0 / torch.sqrt(var + bn.eps)
    # (test_gpu_bn_acc.py: the largest deviation against the largest mean of the tensor - on the hard operands a channel has
    # sigma ~ 750 at |mean| ~ 1, one fp32 ulp of a single z is 3e-5 there, and no fp32 sum holds 2e-6 of that channel's mean)
    e_mu = float((mean.double().cpu() - mu).abs().max() / max(1.0, float(mu.abs().max())))
    e_is = float(((invstd.double().cpu() - ist).abs() / ist).max())
    rm = bn.momentum * mu
    rv = (1 - bn.momentum) + bn.momentum * var * rows / max(rows - 1, 1)
    e_rm = float((bn.running_mean.double().cpu() - rm).abs().max() / max(1.0, float(rm.abs().max())))
    e_rv = float(((bn.running_var.double().cpu() - rv).abs() / rv).max())
    print(f"{opt} {name} {cid}: mean {e_mu:.2e} (2e-6), invstd {e_is:.2e} (3e-7), running_mean {e_rm:.2e} (1e-6), "
          f"running_var {e_rv:.2e} (1e-6)")
    _note(f"{'rows' if pl['route'] else 'tiled'} {opt}: invstd", e_is, 3e-7, cid)
    assert e_mu <= 2e-6 and e_is <= 3e-7 and e_rm <= 1e-6 and e_rv <= 1e-6, f"{opt} {name} {cid}"
    if y is not None:
        yr = (zd - mu) * ist * bn.weight.double().cpu() + bn.bias.double().cpu()
        if res is not None:
            yr = yr + res.double().cpu().reshape(-1, Cn)
        yr = torch.relu(yr)
        e = (y.double().cpu().reshape(-1, Cn) - yr).abs() / yr.abs().clamp_min(1.0)
        assert float(e.max()) <= 2e-5, f"{opt} {name} {cid}: applied output off by {float(e.max()):.2e} at row, channel " \
                                       f"{tuple(int(v) for v in torch.unravel_index(e.argmax(), e.shape))}"


def run_fwd(ops, dev, case, hard, opt, flags):
    inp = inputs(case, hard, dev)
    kind, d, N, H, W, Ci, Co = case
    k, st, pad = geo(kind)
    pl = T.plan(case, flags)
    x, w, res = inp.src, inp.w, inp.res
    b = inp.bias.to(dev) if flags & T.BIAS else None
    ref, mag = inp.ref, inp.mag
    if b is not None:
        ref, mag = ref + b.double(), mag + b.double().abs()
    rows = ref.numel() // Co
    if flags & T.ACC:
        z, acc, info = ops.conv_fwd(x, w, b, st, pad, stats="acc")
        assert info[0] == "acc"
        z32 = inp.get(("z32", b is not None), lambda: in_fp32(ops, lambda: ops.conv_fwd(x, w, b, st, pad)))
        check_conv("z", opt, case, hard, pl, z, z32, ref, mag)
        bn = _Bn(Co, dev)
        bnin = ops.BnAccInput(acc, rows, bn, True)
        y = ops.bn_apply_acc(z, bnin, res, True)
        check_stats("statistics accumulator", opt, case, hard, pl, z, bnin.mean, bnin.invstd, bn, y, res)
    elif flags & T.PARTIALS:
        z, part, info = ops.conv_fwd(x, w, None, st, pad, stats=True)
        z32 = inp.get(("z32", False), lambda: in_fp32(ops, lambda: ops.conv_fwd(x, w, None, st, pad)))
        check_conv("z", opt, case, hard, pl, z, z32, ref, mag)
        assert int(info[2].sum()) == rows, "valid-row counts must add up to the rows"
        bn = _Bn(Co, dev)
        mean, invstd = ops.bn_finalize(part, info, rows, Co, bn.eps, bn.momentum, bn.running_mean, bn.running_var)
        check_stats("partial-sum statistics", opt, case, hard, pl, z, mean, invstd, bn)
    elif flags & T.SCALE:
        sc, sh = inp.scale.to(dev), inp.shift.to(dev)
        f = lambda: ops.conv_fwd(x, w, None, st, pad, scale=sc, shift=sh, residual=res, relu=True)
        check_conv("scale/shift/residual/relu", opt, case, hard, pl, f(), in_fp32(ops, f),
                   torch.relu(ref * sc.double() + sh.double() + res.double()), mag * sc.double().abs() + sh.double().abs() + res.double().abs())
    elif flags & T.RES:
        f = lambda: ops.conv_fwd(x, w, b, st, pad, residual=res)
        check_conv("residual", opt, case, hard, pl, f(), in_fp32(ops, f), ref + res.double(), mag + res.double().abs())
    else:
        f = lambda: ops.conv_fwd(x, w, b, st, pad)
        y = f()
        y32 = inp.get(("z32", b is not None), lambda: in_fp32(ops, f))
        check_conv("bias" if b is not None else "plain", opt, case, hard, pl, y, y32, ref, mag)


def run_dgrad(ops, dev, case, hard, opt, flags):
    inp = inputs(case, hard, dev)
    kind, d, N, H, W, Ci, Co = case
    k, st, pad = geo(kind)
    pl = T.plan(case, flags)
    f = lambda: ops.conv_dgrad(inp.src, inp.w, inp.x_shape, st, pad)
    dx32 = inp.get("dx32", lambda: in_fp32(ops, f))
    if not flags & T.RES:
        check_conv("data gradient", opt, case, hard, pl, f(), dx32, inp.ref, inp.mag)
        return
    dx2 = ops.conv_dgrad(inp.src, inp.w, inp.x_shape, st, pad, residual=inp.res)
    rd = inp.res.double()
    # (fp32 baseline: the exact-fp32 gradient plus one exact-to-half-ulp add)
    check_conv("data gradient + skip gradient", opt, case, hard, pl, dx2, dx32 + inp.res, inp.ref + rd, inp.mag + rd.abs())
    # ... and the RES epilogue is the plain one plus the residual: one more rounding of the sum
    dx = f()
    e = (dx2.double() - (dx.double() + rd)).abs() / (dx.double().abs() + rd.abs()).clamp_min(1e-300)
    assert float(e.max()) <= 2.0 ** -24, f"{opt} {T.case_id(case)}: RES is not plain + residual ({float(e.max()):.3e} of the terms)"


def conv_params():
    out = []
    for case, _ in T.TILED_CASES:
        out += [(case, False, o, f) for o, f in (T.DGRAD_SETS if case[1] else T.FWD_SETS).items()]
    for case in T.HARD_CASES:
        out += [(case, True, o, f) for o, f in (T.DGRAD_SETS if case[1] else T.FWD_SETS).items()]
    for case, _, _ in T.ROW_CASES:
        out += [(case, False, o, f) for o, f in (T.ROWS_DGRAD_SETS if case[1] else T.ROWS_FWD_SETS).items()]
    return out


@pytest.mark.parametrize("case,hard,opt,flags", conv_params(),
                         ids=lambda v: (T.case_id(v) if isinstance(v, tuple) else "hard" if v is True else "" if v is False else str(v)))
def test_case_x_option_set_against_fp64(x6, dev, case, hard, opt, flags):
    (run_dgrad if case[1] else run_fwd)(x6, dev, case, hard, opt, flags)


# ---- weight gradient -----------------------------------------------------------------------------------------------------
def wgrad_operands(case, hard, dev):
    kind, N, H, W, Ci, Co = case
    k, st, pad = geo(kind)
    Ho, Wo = (H, W) if kind == 1 else (H // 2, W // 2)
    g = torch.Generator().manual_seed(sum(case) * 17 + Co)
    if hard:
        # (the products of a weight gradient are summed over all positions: 2^-10..2^10 keeps them inside fp32's exponent range)
        x, dy = hard_operands((N, Ci, H, W), g, -10, 10, 0), hard_operands((N, Co, Ho, Wo), g, -10, 10, 0)
    else:
        x, dy = torch.randn(N, Ci, H, W, generator=g) + 0.5, torch.randn(N, Co, Ho, Wo, generator=g)
    return x, dy, g


def check_wgrad(name, cid, got, got32, ref, mag):
    mag = mag.clamp_min(1e-300)
    r = (got.double().cpu() - ref).abs() / mag
    r32 = float(((got32.double().cpu() - ref).abs() / mag).max())
    bar = min(2e-6, 3 * r32 + 2e-7)
    at = tuple(int(v) for v in torch.unravel_index(r.argmax(), r.shape))
    print(f"wgrad {name} {cid}: error / sum|terms| bf16x6 {float(r.max()):.3e}, exact-fp32 kernel {r32:.3e} (bar {bar:.3e})")
    _note("wgrad", float(r.max()), r32, cid)
    assert torch.isfinite(got).all() and float(r.max()) <= bar, \
        f"wgrad {name} {cid}: {float(r.max()):.3e} > {bar:.3e} at (co, ci, r, s) = {at} (fp32 kernel {r32:.3e})"


@pytest.mark.parametrize("case,hard", [(c, False) for c, *_ in T.WGRAD_CASES] + [(c, True) for c in T.WGRAD_HARD],
                         ids=lambda v: T.case_id(v) if isinstance(v, tuple) else "hard" if v else "")
def test_weight_gradient_against_fp64(x6, dev, case, hard):
    ops = x6
    kind, N, H, W, Ci, Co = case
    k, st, pad = geo(kind)
    cid = T.case_id(case) + ("-hard" if hard else "")
    assert ops.lib().buctd_gconv_wgrad_x6_supported(*case) == 1
    x, dy, g = wgrad_operands(case, hard, dev)
    ref64 = lambda a, b: torch.nn.grad.conv2d_weight(a, (Co, Ci, k, k), b, stride=st, padding=pad)
    ref, mag = ref64(x.double(), dy.double()), ref64(x.double().abs(), dy.double().abs())
    xd, dyd = nhwc(x).to(dev), nhwc(dy).to(dev)
    w_like = wcl(torch.empty(Co, Ci, k, k)).to(dev)
    need = ops.lib().buctd_gconv_wgrad_x6_workspace(*case)
    ops.workspace(need, dev).fill_(0xFF)
    f = lambda: ops.conv_wgrad(xd, dyd, w_like, st, pad)
    dw = f()
    dw32 = in_fp32(ops, f)
    check_wgrad("plain", cid, dw, dw32, ref, mag)
    assert torch.equal(dw, f()), "the weight gradient is not bit-reproducible"
    # accumulate into a non-zero gradient
    out0 = wcl(torch.randn(Co, Ci, k, k, generator=g))
    out = out0.to(dev)
    ops.conv_wgrad(xd, dyd, w_like, st, pad, out=out, accumulate=1)
    check_wgrad("accumulate", cid, out, dw32 + out0.to(dev), ref + out0.double(), mag + out0.double().abs())


# ---- the C interface directly: prepared-image pad, guard bands ----------------------------------------------------------------
def launch(ops, case, flags, src, wp, out, bias=None, res=None, acc=None, part=None, counts=None):
    kind, d, N, H, W, Ci, Co = case
    lib, ptr = ops.lib(), ops.ptr
    assert T.plan(case, flags) is not None
    if d == T.DGRAD:
        rc = lib.buctd_gconv_x6_dgrad(kind, N, H, W, Ci, Co, ptr(src), ptr(wp), ptr(res), ptr(out), ops.stream_ptr())
    elif acc is not None:
        rc = lib.buctd_gconv_x6_fwd_acc(kind, N, H, W, Ci, Co, ptr(src), ptr(wp), ptr(bias), ptr(out), C.c_void_p(acc.ptr),
                                        ops.stream_ptr())
    else:
        rc = lib.buctd_gconv_x6_fwd(kind, N, H, W, Ci, Co, ptr(src), ptr(wp), ptr(bias), None, None, ptr(res), 0, ptr(out),
                                    ptr(part), ptr(counts), ops.stream_ptr())
    ops.check(rc, "gconv_x6 (direct call)")
    return out


@pytest.mark.parametrize("case", T.PAD_CASES, ids=T.case_id)
def test_pad_half_step_of_the_prepared_image(x6, dev, case):
    """Odd nhs: the last K = 32 step has a dead half.  Its products are zero only if the image's pad half-step is finite - the
    image buffer comes from torch.empty, so here it starts as 0xFF bytes (NaN in every bf16 slot)."""
    ops = x6
    kind, d, N, H, W, Ci, Co = case
    k, st, pad = geo(kind)
    assert T.plan(case, 0)["cls"][0][1] % 2 == 1
    inp = inputs(case, False, dev)
    via_ops = ops.conv_dgrad(inp.src, inp.w, inp.x_shape, st, pad) if d else ops.conv_fwd(inp.src, inp.w, None, st, pad)
    nbytes = ops.lib().buctd_gconv_x6_prep_bytes(kind, Ci, Co, d)
    img = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)
    ops.check(ops.lib().buctd_gconv_x6_prep(kind, Ci, Co, ops.ptr(inp.w), d, ops.ptr(img), ops.stream_ptr()), "gconv_x6_prep")
    words = img.view(torch.bfloat16)
    assert torch.isfinite(words.float()).all(), "buctd_gconv_x6_prep leaves slots of the image unwritten"
    got = launch(ops, case, 0, inp.src, img, torch.empty(T.out_shape(case), device=dev))
    assert torch.isfinite(got).all(), f"{case}: the dead half-step leaks into the result"
    assert torch.equal(got, via_ops), f"{case}: differs from the result through ops"


GUARD_SETS = {T.FWD: {"general": T.BIAS, "plain": 0, "STATS": T.ACC, "partials": T.PARTIALS, "RES": T.RES},
              T.DGRAD: {"plain": 0, "RES": T.RES}}
GUARD_PARAMS = [(c, o) for c in T.GUARD_TILED + T.GUARD_ROWS for o, f in GUARD_SETS[c[1]].items()
                if not (c in T.GUARD_ROWS and o == "partials")]


@pytest.mark.parametrize("case,opt", GUARD_PARAMS, ids=lambda v: T.case_id(v) if isinstance(v, tuple) else v)
def test_operands_and_output_between_guard_bands(x6, dev, case, opt):
    """A descriptor range or a row bound that reaches past its tensor reads NaN and shows up in the result; a store past the
    output lands in the sentinel.  Ordinary in-bounds allocations only."""
    ops = x6
    kind, d, N, H, W, Ci, Co = case
    flags = GUARD_SETS[d][opt]
    pl = T.plan(case, flags)
    assert pl["route"] == (1 if case in T.GUARD_ROWS else 0)
    inp = inputs(case, False, dev)
    wp = ops._gconv_prepared(inp.w, kind, d)
    oshape = T.out_shape(case)
    nout = oshape[3]
    shp = (0, 0, max(W, oshape[2]))          # banded() sizes its bands from the width: rows of the wider of the two tensors
    bias = inp.bias.to(dev) if flags & T.BIAS else None

    def run(band):
        ops.step_boundary(dev)
        wrap = (lambda t: banded(t, dev, shp)[0]) if band else (lambda t: t)
        out, big, padn = banded(torch.zeros(oshape, device=dev), dev, shp, SENTINEL) if band else (torch.empty(oshape, device=dev), None, 0)
        acc = ops.AccRef(nout, dev) if flags & T.ACC else None
        part = counts = None
        if flags & T.PARTIALS:
            ng, rpg = C.c_int(), C.c_int()
            assert ops.lib().buctd_gconv_x6_stats_groups(kind, N, H, W, Ci, Co, C.byref(ng), C.byref(rpg)) == 0
            part = torch.zeros((ng.value, nout, 2), device=dev)
            counts = torch.zeros(ng.value, dtype=torch.int32, device=dev)
            if band:
                part, pbig, ppad = banded(part, dev, shp, SENTINEL)
        launch(ops, case, flags, wrap(inp.src), wp, out, bias=bias, res=wrap(inp.res) if flags & T.RES else None, acc=acc,
               part=part, counts=counts)
        res = [out.clone()]
        if band:
            assert untouched(big, padn, out.numel()), f"{opt} {case}: the launch wrote outside its output"
        if acc is not None:
            bnin = ops.BnAccInput(acc, out.numel() // nout, _Bn(nout, dev), True)
            y = ops.bn_apply_acc(res[0], bnin, None, True)       # the consumer decodes the accumulator: mean / invstd exist now
            res += [y, bnin.mean.clone(), bnin.invstd.clone()]
        if part is not None:
            if band:
                assert untouched(pbig, ppad, part.numel()), f"{opt} {case}: the launch wrote outside the partial sums"
            res += [part.clone(), counts.clone()]
        return res

    plain, guarded = run(False), run(True)
    for i, (a, b) in enumerate(zip(plain, guarded)):
        assert torch.isfinite(b.float()).all(), f"{opt} {case}: result {i} picked up a NaN from beyond an operand"
        assert torch.equal(a, b), f"{opt} {case}: result {i} changes with what lies next to the operands"


@pytest.mark.parametrize("case", T.GUARD_WGRAD, ids=T.case_id)
def test_weight_gradient_between_guard_bands(x6, dev, case):
    """operands between NaN bands, dw and the workspace (of exactly the bytes the plan asks for, stale NaNs inside) between
    sentinel bands"""
    ops = x6
    kind, N, H, W, Ci, Co = case
    k, st, pad = geo(kind)
    x, dy, g = wgrad_operands(case, False, dev)
    xd, dyd = nhwc(x).to(dev), nhwc(dy).to(dev)
    w_like = wcl(torch.empty(Co, Ci, k, k)).to(dev)
    plain = ops.conv_wgrad(xd, dyd, w_like, st, pad)
    shp = (0, 0, W)
    need = int(ops.lib().buctd_gconv_wgrad_x6_workspace(*case))
    assert need % 16 == 0
    ws, wbig, wpad = banded(torch.zeros(need // 16, 4, device=dev), dev, shp, SENTINEL)      # (bands of whole 16-byte pieces)
    ws.view(torch.int32).fill_(-1)           # 0xFF bytes: NaN wherever a slab is read before it is written
    dw, big, padn = banded(torch.zeros(Co, k, k, Ci, device=dev), dev, shp, SENTINEL)
    xb, dyb = banded(xd, dev, shp), banded(dyd, dev, shp)        # (named: the allocations must outlive the launch)
    rc = ops.lib().buctd_gconv_wgrad_x6(kind, N, H, W, Ci, Co, ops.ptr(xb[0]), ops.ptr(dyb[0]), ops.ptr(dw), 0, ops.ptr(ws), need,
                                        ops.stream_ptr())
    ops.check(rc, "gconv_wgrad_x6 (direct call)")
    assert untouched(big, padn, dw.numel()), f"wgrad {case}: the launch wrote outside dw"
    assert untouched(wbig, wpad, ws.numel()), f"wgrad {case}: the launch wrote outside its workspace"
    assert torch.isfinite(dw).all(), f"wgrad {case}: picked up a NaN from beyond an operand or from a stale slab"
    assert torch.equal(dw.permute(0, 3, 1, 2), plain), f"wgrad {case}: the result changes with what lies next to the operands"
