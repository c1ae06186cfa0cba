"""Every case of tests/helpers/conv2d_cases.py on the exact-fp32 implicit-GEMM kernels of conv.hip (conv_gemm_kernel,
conv_wgrad_kernel, splitk_reduce_kernel) in the 'fp32' math mode, against an fp64 CPU evaluation of the SAME operation (torch
conv2d / autograd in double on the float inputs), per element.  Before a case runs, buctd_conv2d_plan must report the
implicit-GEMM route and the tile the table names; the host-only closure test (test_conv2d_plan_cover.py) proves that the cases
reach every tile of conv_tile_select and every weight-gradient configuration, split and reduction form.

Metric and bars (none taken from what the kernels give):
  convolution results   |err| / (sum of the absolute values of the element's terms: conv(|x|, |w|) + |bias| ..., likewise for
                        the gradients) <= min(2e-6, (K + 4) * 2^-24), K the reduction length of the element (R*S*Ci forward,
                        R*S*Co data gradient, N*Ho*Wo weight gradient): the worst case of a K-term fp32 fmaf chain with its
                        epilogue, capped by the project's fp32-class bar.  torch's own fp32 convolution on the CPU sits more
                        than 20x inside it; one dropped term is about 1 / K.
  accumulate=1          twice that bar, relative to max(sum |terms|, |base|)
  statistics            bn_finalize of the in-launch Welford partials against fp64 statistics of the device's own z: mean
                        2e-6 * max|z|, invstd 1e-5 relative (the bars of test_gpu_conv_thin.py); y bitwise equal to the plain run
Each convolution bar is asserted on the whole tensor and again on the last row tile, the last column tile (BM / BN of the plan
query), the border pixels and, for the parity-split data gradient, every parity class; the message names the worst element.

Measured on an MI355X (worst |err| / sum|terms| over the cases and option sets of a tile, next to torch's fp32 CPU convolution
on the case that gave it):
  tile                  0         1         2         3 *       4         5         6         7         8         9         10
  forward           2.43e-07  1.32e-07  2.09e-07  7.94e-07  2.59e-07  1.72e-07  2.53e-07  2.34e-07  2.63e-07  2.04e-07  2.57e-07
      torch fp32    2.20e-07  1.68e-07  2.09e-07  3.51e-07  2.77e-07  1.35e-07  2.63e-07  3.54e-08  2.77e-07  1.18e-07  2.83e-07
  data gradient     2.39e-07  1.60e-07  2.35e-07  6.61e-07  3.56e-07  2.02e-07  2.96e-07  2.44e-07  3.13e-07  2.29e-07  2.68e-07
      torch fp32    1.14e-07  1.77e-07  2.10e-07  3.03e-07  3.13e-07  1.17e-07  3.03e-07  3.13e-08  3.31e-07  1.41e-07  2.98e-07
    parity split    -         1.67e-07  2.28e-07  1.74e-07  3.05e-07  1.70e-07  3.32e-07  1.22e-07  2.95e-07  2.11e-07  3.26e-07
      torch fp32    -         1.85e-07  2.28e-07  2.38e-07  2.82e-07  1.34e-07  3.31e-07  1.37e-07  3.36e-07  2.20e-07  3.26e-07
  configuration         0         1         2         3         4
  weight gradient   1.98e-07  1.90e-07  1.77e-07  3.59e-07  2.24e-07
      torch fp32    1.29e-07  2.32e-07  1.78e-07  3.06e-07  2.37e-07
  (* tile 3 holds the hard-operands case, the worst of the module; random-normal cases stay below 3.6e-7.  At the largest
  reduction, K = 3456 on tile 7, the kernel's k-ordered chain gives 2.3e-7 forward and 2.4e-7 data gradient where torch's blocked
  summation gives 3.5e-8 / 3.1e-8: both far inside the bar, a dropped term would be 2.9e-4.)  No case exceeds its bar.
Wall time of the module: 5.6 s (72 tests, fp64 references included; the slowest test takes 1.1 s, most of it the first launch)."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import conv2d_cases as T
from tests.test_gpu_conv3x3_plan_cover import hard_operands

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EPS = 1e-5
SENTINEL = -12345.678
WORST = {}


def bar_of(K):
    return min(2e-6, (K + 4) * U)


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nworst |err| / sum|terms| per direction and tile (kernel / torch fp32 on the CPU, case):")
    for k in sorted(WORST):
        v = WORST[k]
        print(f"  {k[0]:14s} tile {k[1]:2d} par {k[2]}   {v[0]:.2e} / {v[1]:.2e}   at {v[2]}")


@pytest.fixture
def fp32(dev):
    from buctd_amd import ops
    old = ops.get_conv_math()
    ops.set_conv_math("fp32")
    yield ops
    ops.set_conv_math(old)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def wcl(w):
    return w.contiguous(memory_format=torch.channels_last)


def gen(case, salt):
    return torch.Generator().manual_seed(sum(v * (i + 3) for i, v in enumerate(case)) * 7 + salt)


def expect_plan(case, direction, flags, tile, par=0):
    pl = T.plan(case, direction, flags)
    assert pl is not None and pl["route"] == 0 and pl["tile"] == tile and pl["par"] == par, \
        f"{case} direction {direction} flags {flags}: not on the kernel under test: {pl}"
    return pl


def row_subsets(shape, pl):
    """boolean masks over an NHWC result [N, Hr, Wr, OC]: last row tile, last column tile, borders, parity classes"""
    N, Hr, Wr, OC = shape
    BM, BN = pl["BM"], pl["BN"]
    h = torch.arange(Hr).view(1, Hr, 1, 1)
    w = torch.arange(Wr).view(1, 1, Wr, 1)
    full = lambda m: m.expand(N, Hr, Wr, OC)
    sets = {"whole tensor": None}
    if pl["par"]:
        # rows of a parity class are numbered inside the class: pixels (2a + py, 2b + px)
        last = torch.zeros(N, Hr, Wr, 1, dtype=torch.bool)
        for py in (0, 1):
            for px in (0, 1):
                hc, wc = (Hr - py + 1) // 2, (Wr - px + 1) // 2
                if hc * wc == 0:
                    continue
                mc = torch.arange(N * hc * wc).view(N, hc, wc, 1)
                last[:, py::2, px::2] = mc // BM == (N * hc * wc - 1) // BM
                sets[f"parity class ({py}, {px})"] = full((h % 2 == py) & (w % 2 == px))
        sets["last row tile of every class"] = full(last)
    else:
        m = torch.arange(N * Hr * Wr).view(N, Hr, Wr, 1)
        sets["last row tile"] = full(m // BM == (N * Hr * Wr - 1) // BM)
    sets["last column tile"] = full(torch.arange(OC).view(1, 1, 1, OC) // BN == (OC - 1) // BN)
    sets["border pixels"] = full((h == 0) | (h == Hr - 1) | (w == 0) | (w == Wr - 1))
    return sets


def check(direction, name, case, pl, got, ref, mag, K, cpu, subsets, idx="(n, h, w, c)", scale=1.0):
    """got: device result; ref / mag: fp64 value and sum of |terms|; cpu: torch's fp32 result of the same operation or None"""
    mag = mag.clamp_min(1e-300)
    r = (got.double().cpu() - ref).abs() / mag
    bar = scale * bar_of(K)
    r_cpu = float(((cpu.double() - ref).abs() / mag).max()) if cpu is not None else float("nan")
    worst = float(r.max())
    at = tuple(int(v) for v in torch.unravel_index(r.argmax(), r.shape))
    print(f"{direction} {name} {T.case_id(case)}: error / sum|terms| {worst:.3e} at {at} (bar {bar:.3e}, K = {K}; torch fp32 on the CPU "
          f"{r_cpu:.3e}); tile {pl['tile']} {pl['BM']}x{pl['BN']} vec {pl['vec']} par {pl['par']} nsplit {pl['nsplit']}")
    key = (direction, pl["tile"], pl["par"])
    if scale == 1.0 and (key not in WORST or worst > WORST[key][0]):
        WORST[key] = (worst, r_cpu, T.case_id(case) + " " + name)
    assert torch.isfinite(got).all(), f"{direction} {name} {case}: non-finite result"
    for where, m in subsets.items():
        rr = r if m is None else torch.where(m, r, torch.zeros((), dtype=r.dtype))
        w_ = float(rr.max())
        a_ = tuple(int(v) for v in torch.unravel_index(rr.argmax(), rr.shape))
        assert w_ <= bar, (f"{direction} {name} {case} [{where}]: error / sum|terms| {w_:.3e} > {bar:.3e} at {idx} = {a_} "
                           f"(worst of the tensor {worst:.3e} at {at}; torch fp32 on the CPU {r_cpu:.3e}; plan {pl})")


def check_stats(ops, direction, case, pl, z, part, info, rows):
    Cn = z.shape[-1]
    assert part.shape == (-(-rows // pl["BM"]) * pl["WM"], Cn, 2) and info[1] == pl["MF"] * 16
    zd = z.double().cpu().reshape(-1, Cn)
    mu, var = zd.mean(0), zd.var(0, unbiased=False)
    invstd = 1.0 / torch.sqrt(var + EPS)
    mean_d, invstd_d = ops.bn_finalize(part, info, rows, Cn, EPS, 0.1, None, None)
    e_mu = float((mean_d.double().cpu() - mu).abs().max()) / float(zd.abs().max())
    e_is = float(((invstd_d.double().cpu() - invstd).abs() / invstd).max())
    print(f"{direction} statistics {T.case_id(case)}: mean {e_mu:.2e} of max|z| (2e-6), invstd {e_is:.2e} (1e-5)")
    assert e_mu <= 2e-6 and e_is <= 1e-5, f"{direction} statistics {case}: mean {e_mu:.2e}, invstd {e_is:.2e}; plan {pl}"


# ---- forward ---------------------------------------------------------------------------------------------------------------
def run_forward(ops, dev, case, tile, hard):
    N, H, W, Ci, Co, k, s, p = case
    Ho, Wo = T.out_hw(case)
    K, M = k * k * Ci, N * Ho * Wo
    g = gen(case, 1)
    if hard:
        x, w = hard_operands((N, Ci, H, W), g, -20, 20, -14), hard_operands((Co, Ci, k, k), g, -8, 8, -6)
    else:
        x, w = torch.randn(N, Ci, H, W, generator=g) + 0.5, torch.randn(Co, Ci, k, k, generator=g) / math.sqrt(K)
    b, sc, sh = torch.randn(Co, generator=g), torch.rand(Co, generator=g) + 0.5, torch.randn(Co, generator=g)
    res = torch.randn(N, Ho, Wo, Co, generator=g)
    ref = nhwc(F.conv2d(x.double(), w.double(), None, s, p))
    mag = nhwc(F.conv2d(x.double().abs(), w.double().abs(), None, s, p))
    cpu = nhwc(F.conv2d(x, w, None, s, p))
    xd, wd = nhwc(x).to(dev), wcl(w).to(dev)
    pl = expect_plan(case, T.FWD, T.BIAS, tile)
    sub = row_subsets((N, Ho, Wo, Co), pl)
    if hard:
        check("forward", "hard operands", case, pl, ops.conv_fwd(xd, wd, None, s, p), ref, mag, K, cpu, sub)
        return
    bd = b.double()
    y = ops.conv_fwd(xd, wd, b.to(dev), s, p)
    check("forward", "bias", case, pl, y, ref + bd, mag + bd.abs(), K, cpu + b, sub)
    pl2 = expect_plan(case, T.FWD, T.FWD_FLAGS["scale/shift/residual/relu"], tile)
    assert pl2 == pl
    ye = ops.conv_fwd(xd, wd, b.to(dev), s, p, scale=sc.to(dev), shift=sh.to(dev), residual=res.to(dev), relu=True)
    check("forward", "scale/shift/residual/relu", case, pl, ye,
          torch.relu((ref + bd) * sc.double() + sh.double() + res.double()),
          (mag + bd.abs()) * sc.double() + sh.double().abs() + res.double().abs(), K,
          torch.relu((cpu + b) * sc + sh + res), sub)
    assert expect_plan(case, T.FWD, T.FWD_FLAGS["stats"], tile) == pl
    y2, part, info = ops.conv_fwd(xd, wd, b.to(dev), s, p, stats=True)
    assert torch.equal(y2, y), f"forward {case}: the launch with statistics changes y"
    check_stats(ops, "forward", case, pl, y2, part, info, M)


@pytest.mark.parametrize("case,tile", T.FWD_CASES, ids=[T.case_id(c[0]) for c in T.FWD_CASES])
def test_forward_against_fp64(fp32, dev, case, tile):
    run_forward(fp32, dev, case, tile, False)


# ---- data gradient -----------------------------------------------------------------------------------------------------------
def run_dgrad(ops, dev, case, tile, par, hard):
    N, H, W, Ci, Co, k, s, p = case
    Ho, Wo = T.out_hw(case)
    K, M = k * k * Co, N * H * W
    g = gen(case, 2)
    if hard:
        dy, w = hard_operands((N, Co, Ho, Wo), g, -20, 20, -14), hard_operands((Co, Ci, k, k), g, -8, 8, -6)
    else:
        dy, w = torch.randn(N, Co, Ho, Wo, generator=g) + 0.5, torch.randn(Co, Ci, k, k, generator=g) / math.sqrt(K)
    b = torch.randn(Ci, generator=g)
    res = torch.randn(N, H, W, Ci, generator=g)
    opad = (H - ((Ho - 1) * s - 2 * p + k), W - ((Wo - 1) * s - 2 * p + k))
    tr = lambda a, f: nhwc(F.conv_transpose2d(a, f, None, s, p, opad))
    ref, mag, cpu = tr(dy.double(), w.double()), tr(dy.double().abs(), w.double().abs()), tr(dy, w)
    assert ref.shape == (N, H, W, Ci)
    dyd, wd = nhwc(dy).to(dev), wcl(w).to(dev)
    pl = expect_plan(case, T.DGRAD, 0, tile, par)
    sub = row_subsets((N, H, W, Ci), pl)
    dx = ops.conv_dgrad(dyd, wd, (N, H, W, Ci), s, p)
    check("data gradient", "hard operands" if hard else "plain", case, pl, dx, ref, mag, K, cpu, sub)
    if hard:
        return
    # + bias and statistics: the transposed convolution of ConvBnAct; statistics switch the parity split off
    pls = expect_plan(case, T.DGRAD, T.BIAS | T.STATS, tile, 0)
    dxs, part, info = ops.conv_dgrad(dyd, wd, (N, H, W, Ci), s, p, bias=b.to(dev), stats=True)
    check("data gradient", "bias+stats", case, pls, dxs, ref + b.double(), mag + b.double().abs(), K, cpu + b,
          row_subsets((N, H, W, Ci), pls))
    check_stats(ops, "data gradient", case, pls, dxs, part, info, M)
    dxr = ops.conv_dgrad(dyd, wd, (N, H, W, Ci), s, p, residual=res.to(dev))
    check("data gradient", "residual", case, pl, dxr, ref + res.double(), mag + res.double().abs(), K, cpu + res, sub)


@pytest.mark.parametrize("case,tile,par", T.DGRAD_CASES, ids=[T.case_id(c[0]) for c in T.DGRAD_CASES])
def test_data_gradient_against_fp64(fp32, dev, case, tile, par):
    run_dgrad(fp32, dev, case, tile, par, False)


def test_hard_operands(fp32, dev):
    """all 24 mantissa bits set, exponents 2^-20 .. 2^20 inside one reduction: the generator of test_gpu_conv3x3_plan_cover.py,
    whose docstring records 6.1e-7 for this kernel at this shape"""
    case, tile = T.HARD_CASE
    run_forward(fp32, dev, case, tile, True)
    run_dgrad(fp32, dev, case, tile, 0, True)


# ---- weight gradient -----------------------------------------------------------------------------------------------------
def wgrad_autograd(x, dy, wshape, s, p):
    w0 = torch.zeros(wshape, dtype=x.dtype, requires_grad=True)
    F.conv2d(x, w0, None, s, p).backward(dy)
    return w0.grad


def wgrad_subsets(case, pl):
    """over the physical [Co][R][S][Ci] gradient: last tile of output channels, last 64 columns of (r, s, ci)"""
    N, H, W, Ci, Co, k, s, p = case
    ncols = k * k * Ci
    co = torch.arange(Co).view(Co, 1, 1, 1)
    col = torch.arange(ncols).view(1, k, k, Ci)
    return {"whole tensor": None,
            "last row tile": (co // pl["BM"] == (Co - 1) // pl["BM"]).expand(Co, k, k, Ci),
            "last column tile": (col // pl["BN"] == (ncols - 1) // pl["BN"]).expand(Co, k, k, Ci)}


@pytest.mark.parametrize("case,cfg,nsplit", T.WGRAD_CASES, ids=[T.case_id(c[0]) for c in T.WGRAD_CASES])
def test_weight_gradient_against_fp64(fp32, dev, case, cfg, nsplit):
    ops = fp32
    N, H, W, Ci, Co, k, s, p = case
    Ho, Wo = T.out_hw(case)
    K = N * Ho * Wo
    pl = expect_plan(case, T.WGRAD, 0, cfg)
    assert pl["nsplit"] == nsplit
    g = gen(case, 3)
    x, dy = torch.randn(N, Ci, H, W, generator=g) + 0.5, torch.randn(N, Co, Ho, Wo, generator=g)
    phys = lambda t: t.permute(0, 2, 3, 1)          # logical [Co][Ci][R][S] -> the kernel's [Co][R][S][Ci]
    ref = phys(wgrad_autograd(x.double(), dy.double(), (Co, Ci, k, k), s, p))
    mag = phys(wgrad_autograd(x.double().abs(), dy.double().abs(), (Co, Ci, k, k), s, p))
    cpu = phys(wgrad_autograd(x, dy, (Co, Ci, k, k), s, p))
    xd, dyd = nhwc(x).to(dev), nhwc(dy).to(dev)
    w_like = wcl(torch.empty(Co, Ci, k, k)).to(dev)
    d = T.desc(case)
    need = ops.lib().buctd_conv2d_wgrad_workspace(C.byref(d))
    sub = wgrad_subsets(case, pl)

    def run(**kw):
        ops.workspace(need, dev)[:need].fill_(0xFF)        # a slab the kernels do not write reads as NaN
        return ops.conv_wgrad(xd, dyd, w_like, s, p, **kw)

    dw = run()
    check("weight gradient", "plain", case, pl, phys(dw), ref, mag, K, cpu, sub, idx="(co, r, s, ci)")
    assert torch.equal(dw, run()), f"weight gradient {case}: two runs differ"
    base = wcl(torch.randn(Co, Ci, k, k, generator=g))
    out = base.to(dev)
    run(out=out, accumulate=1)
    bs = phys(base).double()
    check("weight gradient", "accumulate", case, pl, phys(out), ref + bs, torch.maximum(mag, bs.abs()), K, None, sub,
          idx="(co, r, s, ci)", scale=2.0)


# ---- guard bands ---------------------------------------------------------------------------------------------------------
def banded(shape, dev):
    """a tensor of `shape` in the middle of a larger sentinel-filled allocation"""
    n = math.prod(shape)
    pad = 4096 + 37
    big = torch.full((2 * pad + n,), SENTINEL, dtype=torch.float32, device=dev)
    return big[pad:pad + n].view(shape), big, pad, n


def assert_banded(what, view, big, pad, n, plain):
    assert bool((big[:pad] == big[0]).all()) and bool((big[pad + n:] == big[-1]).all()) and float(big[0]) == float(big[-1]), \
        f"{what}: the launch wrote outside its output"
    assert not bool((view == big[0]).any()), f"{what}: elements of the output were never written"
    assert torch.equal(view, plain), f"{what}: the result depends on where the output lies"


def test_forward_between_guard_bands(fp32, dev):
    ops = fp32
    case = T.GUARD_FWD
    N, H, W, Ci, Co, k, s, p = case
    Ho, Wo = T.out_hw(case)
    pl = T.plan(case, T.FWD, T.BIAS)
    assert pl["route"] == 0 and pl["vec"] == 0 and (N * Ho * Wo) % pl["BM"] and Co % pl["BN"]
    g = gen(case, 4)
    xd = (torch.randn(N, H, W, Ci, generator=g) + 0.5).to(dev)
    wd = wcl(torch.randn(Co, Ci, k, k, generator=g) / math.sqrt(k * k * Ci)).to(dev)
    bd = torch.randn(Co, generator=g).to(dev)
    plain = ops.conv_fwd(xd, wd, bd, s, p)
    y, big, pad, n = banded((N, Ho, Wo, Co), dev)
    d = T.desc(case)
    ops.check(ops.lib().buctd_conv2d_fwd(C.byref(d), ops.ptr(xd), ops.ptr(wd), ops.ptr(bd), None, None, None, 0, ops.ptr(y), None,
                                         ops.stream_ptr()), "conv2d_fwd")
    assert_banded(f"forward {case}", y, big, pad, n, plain)


def test_parity_data_gradient_between_guard_bands(fp32, dev):
    ops = fp32
    case = T.GUARD_DGRAD
    N, H, W, Ci, Co, k, s, p = case
    Ho, Wo = T.out_hw(case)
    pl = T.plan(case, T.DGRAD, 0)
    assert pl["route"] == 0 and pl["par"] == 1 and H % 2 and W % 2
    g = gen(case, 5)
    dyd = (torch.randn(N, Ho, Wo, Co, generator=g) + 0.5).to(dev)
    wd = wcl(torch.randn(Co, Ci, k, k, generator=g) / math.sqrt(k * k * Co)).to(dev)
    plain = ops.conv_dgrad(dyd, wd, (N, H, W, Ci), s, p)
    dx, big, pad, n = banded((N, H, W, Ci), dev)
    d = T.desc(case)
    ops.check(ops.lib().buctd_conv2d_dgrad(C.byref(d), ops.ptr(dyd), ops.ptr(wd), None, ops.ptr(dx), None, ops.stream_ptr()),
              "conv2d_dgrad")
    assert_banded(f"data gradient {case}", dx, big, pad, n, plain)


def test_split_weight_gradient_between_guard_bands(fp32, dev):
    ops = fp32
    case = T.GUARD_WGRAD
    N, H, W, Ci, Co, k, s, p = case
    Ho, Wo = T.out_hw(case)
    pl = T.plan(case, T.WGRAD)
    assert pl["route"] == 0 and pl["nsplit"] > 1 and (N * Ho * Wo) % pl["pix_per_split"] and Co % pl["BM"] and (k * k * Ci) % pl["BN"]
    g = gen(case, 6)
    xd = (torch.randn(N, H, W, Ci, generator=g) + 0.5).to(dev)
    dyd = torch.randn(N, Ho, Wo, Co, generator=g).to(dev)
    w_like = wcl(torch.empty(Co, Ci, k, k)).to(dev)
    d = T.desc(case)
    need = ops.lib().buctd_conv2d_wgrad_workspace(C.byref(d))
    plain = ops.conv_wgrad(xd, dyd, w_like, s, p).permute(0, 2, 3, 1)       # the physical [Co][R][S][Ci]
    # the slabs, too, between sentinels: a split that writes past its slab or the last slab lands in them
    ws, wbig, wpad, wn = banded((need // 4,), dev)
    dw, big, pad, n = banded((Co, k, k, Ci), dev)
    ops.check(ops.lib().buctd_conv2d_wgrad(C.byref(d), ops.ptr(xd), ops.ptr(dyd), ops.ptr(dw), 0, ops.ptr(ws), need, ops.stream_ptr()),
              "conv2d_wgrad")
    assert_banded(f"weight gradient {case}", dw, big, pad, n, plain)
    assert bool((wbig[:wpad] == wbig[0]).all()) and bool((wbig[wpad + wn:] == wbig[-1]).all()), "a split wrote outside the workspace"
    assert not bool((ws == wbig[0]).any()), "elements of the slabs were never written"
