"""Every case of tests/helpers/c3_cases.py x every option set of the 3x3 bf16x6 convolution against an fp64 CPU evaluation of
the SAME operation (torch conv2d / autograd in double on the float inputs), per element.  The host-only closure test
(test_conv3x3_plan_cover.py) proves that the cases reach every tile plan and every train-mode kernel variant.

Metrics and bars (none of them taken from what the kernels give):
  convolution outputs   |err| / (sum of the absolute values of the terms of the element: conv(|x|, |w|) + |bias| ...), the
                        yardstick of test_bf16x6_split_is_exact_on_hard_operands, with its bar: <= 2e-6 and <= 3 x (the same
                        ratio of the exact-fp32 kernel on the same inputs) + 2e-7;
  forward statistics    the bars of test_gpu_bn_acc.py (mean 2e-6 max(1, |mu|), invstd 3e-7, running_var 1e-6 relative, applied
                        output 2e-5 max(1, |y|)), fp64 statistics of the device's own z;
  BatchNorm-backward    the sums s1 = sum m g, s2 = sum m g zhat (read back as dbeta / dgamma from the kernel that consumes the
  sums, dz              accumulator) and dz against autograd of an fp64 BatchNorm + ReLU on the device's own g: <= max(5e-6,
                        4 x the distance of the same evaluation in fp32 on the CPU) relative to the largest element - the rule
                        of _check in test_gpu_blocks.py.
Each convolution bar is asserted on the whole tensor and again on the last position tile, the last column tile (BM / BN of
the plan query) and the border pixels, and the message names the worst element (n, h, w, c).

Measured on an MI355X: worst figure per option set over all 36 cases, next to the baseline it was judged against (the
exact-fp32 kernel's ratio for the convolution outputs, the fp32 CPU evaluation for the BatchNorm-backward quantities; the worst
convolution ratios all come from the hard-operands case, random-normal cases stay below 2e-7):
  option set    conv ratio / fp32 kernel   invstd (bar 3e-7)   s1 / fp32 CPU        s2 / fp32 CPU        dz / fp32 CPU
  general       7.96e-07 / 6.11e-07        8.3e-08
  STATS         7.96e-07 / 6.11e-07        1.2e-07
  STATS|IN_BN   4.47e-07 / 3.84e-07        9.7e-08
  RES           6.28e-07 / 6.80e-07
  BS_REBUILD    6.06e-07 / 6.62e-07                            7.4e-08 / 1.0e-07    9.9e-08 / 9.3e-08    1.7e-07 / 1.1e-07
  RES|BS_Y      6.28e-07 / 6.80e-07                            1.1e-07 / 9.1e-08    1.2e-07 / 1.1e-07    1.8e-07 / 1.3e-07
  wgrad         3.78e-07 / 7.38e-07
(every BatchNorm-backward figure is below the 5e-6 floor of its bar).  Wall time of the module: 45-52 s (255 tests; test_gpu_conv3x3_split.py:
6 s on the same machine - the difference is the twelve model shapes at batch 32 and their fp64 references)."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import c3_cases as T
from tests.helpers.c3_checks import (CONV_CASES, HARD, WORST, Inputs, _Bn, _id, bn_params, bnstat_acc, check_bn_backward, check_conv,
                                     check_stats, check_wgrad, hard_operands, in_fp32, inputs, nchw, nhwc, rebuilt_mask, wcl,
                                     wgrad_ref)
from tests.helpers.guard_bands import SENTINEL, banded, untouched

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nworst figures per option set (measured / baseline, case):")
    for k in sorted(WORST):
        v = WORST[k]
        print(f"  {k:28s} {v[0]:.3e} / {v[1]:.3e}  at {v[2]}")



@pytest.fixture
def x6(dev):
    from buctd_amd import ops
    old = ops.get_conv_math()
    ops.set_conv_math("bf16x6")
    ops.step_boundary(dev)
    yield ops
    ops.set_conv_math(old)


def run_general(ops, dev, case):
    inp = inputs(case)
    N, H, W, Ci, Co = inp.shape
    xd, wd, wbd = nhwc(inp.x).to(dev), wcl(inp.w).to(dev), wcl(inp.wb).to(dev)
    resd = nhwc(inp.res).to(dev)
    ref, mag = inp.fwd()
    b, sc, sh = inp.bias.to(dev), inp.scale.to(dev), inp.shift.to(dev)
    f = lambda: ops.conv_fwd(xd, wd, b, 1, 1)
    check_conv("bias", "general", case, f(), in_fp32(ops, f), ref + inp.bias.double(), mag + inp.bias.double().abs())
    f = lambda: ops.conv_fwd(xd, wd, None, 1, 1, scale=sc, shift=sh, residual=resd, relu=True)
    rd = nhwc(inp.res).double()
    check_conv("scale/shift/residual/relu", "general", case, f(), in_fp32(ops, f),
               torch.relu(ref * inp.scale.double() + inp.shift.double() + rd),
               mag * inp.scale.double().abs() + inp.shift.double().abs() + rd.abs())
    z, part, info = ops.conv_fwd(xd, wd, None, 1, 1, stats=True)
    z32 = inp.get("z32", lambda: in_fp32(ops, lambda: ops.conv_fwd(xd, wd, None, 1, 1)).cpu())
    check_conv("partial-sum statistics: z", "general", case, z, z32, ref, mag)
    assert int(info[2].sum()) == N * H * W, "valid-row counts must add up to N*H*W"
    bn = _Bn(Co, dev)

    class St:
        pass
    st = St()
    st.mean, st.invstd = ops.bn_finalize(part, info, N * H * W, Co, bn.eps, bn.momentum, bn.running_mean, bn.running_var)
    check_stats("partial-sum statistics", "general", case, z, st, bn)
    f = lambda: ops.conv_dgrad(xd, wbd, (N, H, W, Co), 1, 1)
    dref, dmag = inp.dgrad()
    dx32 = inp.get("dx32", lambda: in_fp32(ops, f).cpu())
    check_conv("data gradient", "general", case, f(), dx32, dref, dmag)


def run_stats(ops, dev, case):
    inp = inputs(case)
    N, H, W, Ci, Co = inp.shape
    xd, wd = nhwc(inp.x).to(dev), wcl(inp.w).to(dev)
    ref, mag = inp.fwd()
    z, acc, info = ops.conv_fwd(xd, wd, None, 1, 1, stats="acc")
    assert info[0] == "acc"
    z32 = inp.get("z32", lambda: in_fp32(ops, lambda: ops.conv_fwd(xd, wd, None, 1, 1)).cpu())
    check_conv("z", "STATS", case, z, z32, ref, mag)
    bn = _Bn(Co, dev)
    bnin = ops.BnAccInput(acc, N * H * W, bn, True)
    resd = nhwc(inp.res).to(dev)
    y = ops.bn_apply_acc(z, bnin, resd, True)
    check_stats("statistics", "STATS", case, z, bnin, bn, y, resd)


def run_stats_in_bn(ops, dev, case):
    inp = inputs(case)
    N, H, W, Ci, Co = inp.shape
    g = torch.Generator().manual_seed(Ci + 11)
    w0 = (hard_operands((Ci, Ci, 3, 3), g, -8, 8, -6) if inp.hard else torch.randn(Ci, Ci, 3, 3, generator=g) / math.sqrt(9 * Ci))
    # the producer: a convolution with its own statistics accumulator; its raw output z1 is this launch's input
    z1, acc1, info1 = ops.conv_fwd(nhwc(inp.x).to(dev), wcl(w0).to(dev), None, 1, 1, stats="acc")
    assert info1[0] == "acc"
    bn1 = _Bn(Ci, dev, seed=1)
    bnin1 = ops.BnAccInput(acc1, N * H * W, bn1, True, relu=True)
    wd = wcl(inp.w).to(dev)
    z2, acc2, info2 = ops.conv_fwd(z1, wd, None, 1, 1, stats="acc", in_bn=bnin1)
    assert info2[0] == "acc"
    # fp64: conv(relu(bn_train(z1))) from the same z1
    zd = z1.double().cpu()
    z2d = zd.reshape(-1, Ci)
    mu, var = z2d.mean(0), z2d.var(0, unbiased=False)
    a = (zd - mu) / torch.sqrt(var + bn1.eps) * bn1.weight.double().cpu()
    beta = bn1.bias.double().cpu()
    y1 = torch.relu(a + beta)
    terms = torch.where(y1 > 0, a.abs() + beta.abs(), torch.zeros((), dtype=torch.float64))
    w64 = inp.w.double()
    ref = nhwc(F.conv2d(nchw(y1), w64, None, 1, 1))
    mag = nhwc(F.conv2d(nchw(terms), w64.abs(), None, 1, 1))
    y1f = y1.float().to(dev)
    z32 = in_fp32(ops, lambda: ops.conv_fwd(y1f, wd, None, 1, 1))
    check_conv("z of conv(relu(bn(z1)))", "STATS|IN_BN", case, z2, z32, ref, mag)
    check_stats("the producer's statistics (mean_out, invstd_out, running)", "STATS|IN_BN", case, z1, bnin1, bn1)
    bn2 = _Bn(Co, dev, seed=2)
    bnin2 = ops.BnAccInput(acc2, N * H * W, bn2, True)
    y = ops.bn_apply_acc(z2, bnin2, None, True)
    check_stats("its own statistics", "STATS|IN_BN", case, z2, bnin2, bn2, y)


def run_res(ops, dev, case):
    inp = inputs(case)
    N, H, W, Ci, Co = inp.shape
    xd, wbd, resd = nhwc(inp.x).to(dev), wcl(inp.wb).to(dev), nhwc(inp.res).to(dev)
    f = lambda: ops.conv_dgrad(xd, wbd, (N, H, W, Co), 1, 1, residual=resd)
    dref, dmag = inp.dgrad()
    rd = nhwc(inp.res).double()
    check_conv("data gradient + skip gradient", "RES", case, f(), in_fp32(ops, f), dref + rd, dmag + rd.abs())


def run_bs(ops, dev, case, opt):
    inp = inputs(case)
    N, H, W, Ci, Co = inp.shape
    with_y = opt == "RES|BS_Y"
    xd, wbd = nhwc(inp.x).to(dev), wcl(inp.wb).to(dev)
    mean, invstd, gamma, beta = bn_params(inp, dev)
    dref, dmag = inp.dgrad()
    dx32 = inp.get("dx32", lambda: in_fp32(ops, lambda: ops.conv_dgrad(xd, wbd, (N, H, W, Co), 1, 1)).cpu())
    if with_y:
        # the forward output of that BatchNorm (with its skip connection) decides the mask; the skip gradient joins dx
        yb = torch.relu(((inp.zb.double() - mean.double()) * (invstd.double() * gamma.double()) + beta.double()
                         + inp.r2.double())).float()
        m, res_bn = yb > 0, inp.r2
        rd = nhwc(inp.res)
        dref, dmag, dx32 = dref + rd.double(), dmag + rd.double().abs(), dx32 + rd      # (fp32: one exact-to-half-ulp add)
        resd, ybd, betad = rd.to(dev), yb.to(dev), None
    else:
        m, res_bn = rebuilt_mask(ops, inp, mean, invstd, gamma, beta, dev), None
        resd, ybd, betad = None, None, beta.to(dev)
    dx = torch.empty((N, H, W, Co), device=dev)
    dz, dgamma, dbeta = bnstat_acc(ops, inp.shape, xd, wbd, resd, dx, inp.zb.to(dev), ybd, mean.to(dev), invstd.to(dev),
                                   gamma.to(dev), betad)
    check_conv("dx", opt, case, dx, dx32, dref, dmag)
    check_bn_backward(opt, case, dx, dz, dgamma, dbeta, inp.zb, res_bn, gamma, beta, m)


RUN = {"general": run_general, "STATS": run_stats, "STATS|IN_BN": run_stats_in_bn, "RES": run_res,
       "BS_REBUILD": lambda ops, dev, case: run_bs(ops, dev, case, "BS_REBUILD"),
       "RES|BS_Y": lambda ops, dev, case: run_bs(ops, dev, case, "RES|BS_Y")}


@pytest.mark.parametrize("opt", list(T.OPTION_SETS))
@pytest.mark.parametrize("case", CONV_CASES, ids=_id)
def test_case_x_option_set_against_fp64(x6, dev, case, opt):
    RUN[opt](x6, dev, case)


# ---- weight gradient -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(s, False) for s in T.WGRAD_CASES] + [(HARD, True)], ids=_id)
def test_weight_gradient_against_fp64(x6, dev, case):
    ops = x6
    shape, hard = case
    N, H, W, Ci, Co = shape
    from buctd_amd import _C
    wpl = (C.c_int * 4)()
    assert _C.lib().buctd_conv3x3_wgrad_bf16x6_plan(*shape, wpl) == 0
    g = torch.Generator().manual_seed(sum(shape) * 17 + Co)
    if hard:
        # (the products of a weight gradient are summed over all positions: 2^-10..2^10 keeps them inside fp32's exponent range)
        x, dy = hard_operands((N, Ci, H, W), g, -10, 10, 0), hard_operands((N, Co, H, W), g, -10, 10, 0)
    else:
        x, dy = torch.randn(N, Ci, H, W, generator=g) + 0.5, torch.randn(N, Co, H, W, generator=g)
    w_like = wcl(torch.empty(Co, Ci, 3, 3)).to(dev)
    xd, dyd = nhwc(x).to(dev), nhwc(dy).to(dev)
    ref, mag = wgrad_ref(x.double(), dy.double(), shape), wgrad_ref(x.double().abs(), dy.double().abs(), shape)
    need = ops.lib().buctd_conv3x3_wgrad_bf16x6_workspace(*shape)
    ops.workspace(need, dev).fill_(0xFF)
    f = lambda: ops.conv_wgrad(xd, dyd, w_like, 1, 1)
    dw = f()
    dw32 = in_fp32(ops, f)
    check_wgrad("plain", case, dw, dw32, ref, mag)
    assert torch.equal(dw, f()), "the weight gradient is not bit-reproducible"
    # accumulate into a non-zero gradient
    out0 = wcl(torch.randn(Co, Ci, 3, 3, generator=g))
    out = out0.to(dev)
    ops.conv_wgrad(xd, dyd, w_like, 1, 1, out=out, accumulate=1)
    check_wgrad("accumulate", case, out, dw32 + out0.to(dev), ref + out0.double(), mag + out0.double().abs())
    # the X operand normalised on the fly: x is a raw z, the kernel uses relu((z - mean) (invstd gamma) + beta)
    zd = x.double()
    mean = zd.mean((0, 2, 3)).float()
    invstd = (1.0 / torch.sqrt(zd.var((0, 2, 3), unbiased=False) + 1e-5)).float()
    bn = _Bn(Ci, dev, seed=4)
    x_bn = (mean.to(dev), invstd.to(dev), bn.weight, bn.bias, True)
    if Ci % (wpl[0] * 16) != 0:
        with pytest.raises(_C.BuctdHipError):        # documented: the fused input BatchNorm needs whole channel chunks
            ops.conv_wgrad(xd, dyd, w_like, 1, 1, x_bn=x_bn)
        return
    v = lambda t: t.double().cpu().view(1, -1, 1, 1)
    a = (zd - v(mean)) * (v(invstd) * v(bn.weight))
    y1 = torch.relu(a + v(bn.bias))
    terms = torch.where(y1 > 0, a.abs() + v(bn.bias).abs(), torch.zeros((), dtype=torch.float64))
    y1f = nhwc(y1.float()).to(dev)
    dwb = ops.conv_wgrad(xd, dyd, w_like, 1, 1, x_bn=x_bn)
    dwb32 = in_fp32(ops, lambda: ops.conv_wgrad(y1f, dyd, w_like, 1, 1))
    check_wgrad("x_bn", case, dwb, dwb32, wgrad_ref(y1, dy.double(), shape), wgrad_ref(terms, dy.double().abs(), shape))
    assert torch.equal(dwb, ops.conv_wgrad(xd, dyd, w_like, 1, 1, x_bn=x_bn))


# ---- guard bands -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", [o for o in T.OPTION_SETS if o != "general"])
@pytest.mark.parametrize("shape", T.GUARD_CASES, ids=T.case_id)
def test_inputs_between_nan_bands(x6, dev, shape, opt):
    """A descriptor range or a row bound that reaches past its tensor reads NaN and shows up in the result; a store past the
    output lands in the sentinel.  Ordinary in-bounds allocations only."""
    ops = x6
    N, H, W, Ci, Co = shape
    inp = Inputs(shape, False)
    xd, resd = nhwc(inp.x).to(dev), nhwc(inp.res).to(dev)
    zbd, r2 = inp.zb.to(dev), inp.r2
    mean, invstd, gamma, beta = (t.to(dev) for t in bn_params(inp, dev))

    def run(band):
        ops.step_boundary(dev)
        wrap = (lambda t: banded(t, dev, shape)[0]) if band else (lambda t: t)
        if opt == "STATS":
            z, acc, _ = ops.conv_fwd(wrap(xd), wcl(inp.w).to(dev), None, 1, 1, stats="acc")
            bnin = ops.BnAccInput(acc, N * H * W, _Bn(Co, dev), True)
            return z, ops.bn_apply_acc(z, bnin, None, True), bnin.mean.clone()
        if opt == "STATS|IN_BN":
            g = torch.Generator().manual_seed(5)
            w0 = wcl(torch.randn(Ci, Ci, 3, 3, generator=g) / math.sqrt(9 * Ci)).to(dev)
            z1, acc1, _ = ops.conv_fwd(xd, w0, None, 1, 1, stats="acc")
            bnin1 = ops.BnAccInput(acc1, N * H * W, _Bn(Ci, dev, seed=1), True, relu=True)
            z2, acc2, _ = ops.conv_fwd(wrap(z1), wcl(inp.w).to(dev), None, 1, 1, stats="acc", in_bn=bnin1)
            bnin2 = ops.BnAccInput(acc2, N * H * W, _Bn(Co, dev, seed=2), True)
            return z2, ops.bn_apply_acc(z2, bnin2, None, True), bnin1.invstd.clone()
        wbd = wcl(inp.wb).to(dev)
        if opt == "RES":
            return (ops.conv_dgrad(wrap(xd), wbd, (N, H, W, Co), 1, 1, residual=wrap(resd)),)
        with_y = opt == "RES|BS_Y"
        yb = torch.relu(ops.bn_apply(zbd, mean, invstd, gamma, beta, None, False) + r2.to(dev)) if with_y else None
        dx, big, pad = banded(torch.zeros((N, H, W, Co), device=dev), dev, shape, SENTINEL) if band else \
            (torch.empty((N, H, W, Co), device=dev), None, 0)
        out = bnstat_acc(ops, shape, wrap(xd), wbd, wrap(resd) if with_y else None, dx, wrap(zbd), wrap(yb) if with_y else None,
                         mean, invstd, gamma, None if with_y else beta)
        if band:
            assert untouched(big, pad, dx.numel()), f"{opt} {shape}: the launch wrote outside dx"
        return (dx.clone(),) + out

    plain, guarded = run(False), run(True)
    for i, (a, b) in enumerate(zip(plain, guarded)):
        assert torch.isfinite(b).all(), f"{opt} {shape}: result {i} picked up a NaN from beyond an input tensor"
        assert torch.equal(a, b), f"{opt} {shape}: result {i} changes with what lies next to the inputs"


@pytest.mark.parametrize("form", ["plain", "x_bn"])
@pytest.mark.parametrize("shape", T.GUARD_WGRAD_CASES, ids=T.case_id)
def test_weight_gradient_between_nan_bands(x6, dev, shape, form):
    ops = x6
    N, H, W, Ci, Co = shape
    g = torch.Generator().manual_seed(sum(shape))
    xd = (torch.randn(N, H, W, Ci, generator=g) + 0.5).to(dev)
    dyd = torch.randn(N, H, W, Co, generator=g).to(dev)
    bn = _Bn(Ci, dev, seed=4)
    x_bn = (torch.full((Ci,), 0.5, device=dev), torch.full((Ci,), 1.1, device=dev), bn.weight, bn.bias, True) if form == "x_bn" else None
    w_like = wcl(torch.empty(Co, Ci, 3, 3)).to(dev)
    need = ops.lib().buctd_conv3x3_wgrad_bf16x6_workspace(*shape)
    ops.workspace(need, dev).fill_(0xFF)
    plain = ops.conv_wgrad(xd, dyd, w_like, 1, 1, x_bn=x_bn)
    ops.workspace(need, dev).fill_(0xFF)
    out, big, pad = banded(wcl(torch.zeros(Co, Ci, 3, 3)).to(dev).permute(0, 2, 3, 1), dev, shape, SENTINEL)
    out = out.permute(0, 3, 1, 2)          # logical [Co][Ci][3][3] over the physical [Co][3][3][Ci] inside the sentinel
    got = ops.conv_wgrad(banded(xd, dev, shape)[0], banded(dyd, dev, shape)[0], w_like, 1, 1, out=out, accumulate=0, x_bn=x_bn)
    assert untouched(big, pad, out.numel()), f"wgrad {shape}: the launch wrote outside dw"
    assert torch.isfinite(got).all(), f"wgrad {shape}: picked up a NaN from beyond an operand"
    assert torch.equal(got, plain), f"wgrad {shape}: the result changes with what lies next to the operands"
