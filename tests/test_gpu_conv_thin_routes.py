"""Every case of tests/helpers/conv_thin_cases.py on the nine thin-channel kernels of conv.hip (conv_fwd_thin_kernel,
conv_fwd_thin_px4_kernel, conv_dgrad_thin_kernel, conv_dgrad_thin_px4_kernel, conv_dgrad_thin_s2_kernel,
conv3x3_thin_in_fwd_kernel, conv3x3_thin_in_wgrad_kernel, conv_wgrad_thin_kernel, conv_wgrad_thin_rows_kernel) in the 'fp32'
math mode, against an fp64 CPU evaluation of the SAME operation (torch conv2d / autograd in double on the float inputs), per
element.  Before a case runs, buctd_conv2d_plan must report the thin route the table names (and, for a weight gradient, its
nsplit); the host-only closure test (test_conv_thin_plan_cover.py) proves that the cases reach every instance, loop and ragged
branch of these kernels that the routing can pick.  test_gpu_conv_thin.py stays as the check at the model's shapes.

Metric and bars (those of test_gpu_conv2d_fp32.py; none taken from what the kernels give):
  convolution results   |err| / (sum of the absolute values of the element's terms: conv(|x|, |w|) + |bias|, likewise for the
                        gradients) <= min(2e-6, (K + 4) * 2^-24), K the reduction length of the element (k*k*Ci forward,
                        k*k*Co data gradient, N*Ho*Wo weight gradient)
  accumulate=1          twice that bar, relative to max(sum |terms|, |base|); the same for a loop case against the sum of two
                        half-batch calls (each below the workgroup cap) through accumulate=1
  statistics            bn_finalize of the in-launch partials against fp64 statistics of the device's own y: mean
                        2e-6 * max|y|, invstd 1e-5 relative; y bitwise equal to the run without statistics
Each forward / data-gradient bar is asserted on the whole tensor and again on the last row tile, the last column tile (the
tile of the route under test), the one-pixel image border and, for 7x7 filters, the 3-pixel border; each weight-gradient bar on
the whole tensor, the outer taps (whose halo reaches farthest) and the last four channels of the wide side.  The message names
the worst element.  A weight gradient runs with accumulate=0 into a NaN-filled gradient over a NaN-filled workspace, a second
time (bitwise equal: no atomics), and with accumulate=1 onto a random base.

Measured on an MI355X (worst |err| / sum|terms| over the cases of a route, next to torch's fp32 CPU result on the case that
gave it; 'hard' = the hard-operands case of the route):
  route                     1          2          3          4
  forward               2.13e-07   1.33e-07   2.72e-07   3.54e-07
      torch fp32        2.13e-07   2.00e-07   1.96e-07   2.56e-07
    hard                4.94e-07   5.50e-07   8.98e-07   4.52e-07
      torch fp32        5.02e-07   2.98e-07   8.40e-07   4.52e-07
  data gradient         2.59e-07   2.55e-07   3.35e-07   4.13e-07
      torch fp32        2.59e-07   1.56e-07   3.35e-07   4.13e-07
    hard                3.98e-07   4.99e-07   8.56e-07   7.40e-07
      torch fp32        3.98e-07   5.67e-07   8.56e-07   7.40e-07
  weight gradient       5.13e-08   3.11e-08   3.07e-08
      torch fp32        8.93e-08   7.91e-08   4.52e-08
  (the bar is 2e-6 for every case but the thin-input ones with K = 9, 18 and 27: 7.7e-7, 1.3e-6 and 1.8e-6.  The loop cases
  agree with the sum of their two half-batch calls to 2.1e-8; in-launch statistics: mean within 2.3e-8 of max|y|, invstd
  within 3.3e-7.)
No case exceeds its bar, on any subset; the kernels needed no change.
Wall time of the module: 12.1 s (182 tests, fp64 references included; the slowest test takes 1.1 s, most of it the first launch,
the slowest after it 0.75 s)."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import conv_thin_cases as T
from tests.helpers.guard_bands import Bands
from tests.test_gpu_conv3x3_plan_cover import hard_operands

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EPS = 1e-5
DIRS = {T.FWD: "forward", T.DGRAD: "data gradient", T.WGRAD: "weight gradient"}
WORST = {}


def bar_of(K):
    return min(2e-6, (K + 4) * U)


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nworst |err| / sum|terms| per direction and route (kernel / torch fp32 on the CPU, case):")
    for k in sorted(WORST):
        v = WORST[k]
        print(f"  {DIRS[k[0]]:15s} route {k[1]} {k[2]:13s}  {v[0]:.2e} / {v[1]:.2e}   at {v[2]}")


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


def phys(t):
    """logical [Co][Ci][R][S] -> the kernels' [Co][R][S][Ci]"""
    return t.permute(0, 2, 3, 1)


def gen(case, salt):
    return torch.Generator().manual_seed(sum(v * (i + 3) for i, v in enumerate(case)) * 7 + salt)


def ids(cases):
    return [f"r{c[1]}-{T.case_id(c[0])}" for c in cases]


def expect_plan(case, direction, flags, route, nsplit=None):
    pl = T.plan(case, direction, flags)
    assert pl is not None and pl["route"] == route and (nsplit is None or pl["nsplit"] == nsplit), \
        f"{DIRS[direction]} {case} flags {flags}: not on the kernel under test (route {route}, nsplit {nsplit}): {pl}"
    return pl


def pixel_subsets(shape, tile, k):
    """boolean masks over an NHWC result: last row tile, last column tile, borders"""
    N, Hr, Wr, OC = shape
    TH, TW = tile
    h = torch.arange(Hr).view(1, Hr, 1, 1)
    w = torch.arange(Wr).view(1, 1, Wr, 1)
    full = lambda m: m.expand(N, Hr, Wr, OC)
    sets = {"whole tensor": None}
    if TH == 0:         # TW pixels of the flat [N][H][W] order per workgroup
        m = torch.arange(N * Hr * Wr).view(N, Hr, Wr, 1)
        sets["last workgroup"] = full(m // TW == (N * Hr * Wr - 1) // TW)
    else:
        sets["last row tile"] = full(h // TH == (Hr - 1) // TH)
        sets["last column tile"] = full(w // TW == (Wr - 1) // TW)
    border = lambda b: full((h < b) | (h >= Hr - b) | (w < b) | (w >= Wr - b))
    sets["one-pixel border"] = border(1)
    if k == 7:
        sets["3-pixel border"] = border(3)
    return sets


def wgrad_subsets(case):
    """over the physical [Co][R][S][Ci] gradient"""
    N, H, W, Ci, Co, k, s, p = case
    r = torch.arange(k).view(1, k, 1, 1)
    sx = torch.arange(k).view(1, 1, k, 1)
    co = torch.arange(Co).view(Co, 1, 1, 1)
    ci = torch.arange(Ci).view(1, 1, 1, Ci)
    full = lambda m: m.expand(Co, k, k, Ci)
    wide = full(co >= (Co - 1) // 4 * 4) if Co > Ci else full(ci >= (Ci - 1) // 4 * 4)
    return {"whole tensor": None, "outer taps": full((r == 0) | (r == k - 1) | (sx == 0) | (sx == k - 1)),
            "last four channels of the wide side": wide}


def check(direction, route, name, case, got, ref, mag, K, cpu, subsets, idx="(n, y, x, c)", scale=1.0, flags=0):
    """got: device result; ref / mag: fp64 value and sum of |terms|; cpu: torch's fp32 result of the same operation or None"""
    mag = mag.clamp_min(1e-300)
    r = (got.double().cpu() - ref).abs() / mag
    bar = scale * bar_of(K)
    r_cpu = float(((cpu.double() - ref).abs() / mag).max()) if cpu is not None else float("nan")
    worst = float(r.max())
    at = tuple(int(v) for v in torch.unravel_index(r.argmax(), r.shape))
    what = f"{DIRS[direction]} route {route} [{' / '.join(T.key(case, direction, route, flags))}] {name} {T.case_id(case)}"
    print(f"{what}: error / sum|terms| {worst:.3e} at {at} (bar {bar:.3e}, K = {K}; torch fp32 on the CPU {r_cpu:.3e})")
    key = (direction, route, "hard operands" if name == "hard operands" else "")
    if scale == 1.0 and (key not in WORST or worst > WORST[key][0]):
        WORST[key] = (worst, r_cpu, T.case_id(case) + " " + name)
    assert torch.isfinite(got).all(), f"{what}: non-finite result"
    for where, m in subsets.items():
        rr = r if m is None else torch.where(m, r, torch.zeros((), dtype=r.dtype))
        w_ = float(rr.max())
        a_ = tuple(int(v) for v in torch.unravel_index(rr.argmax(), rr.shape))
        assert w_ <= bar, (f"{what} [{where}]: error / sum|terms| {w_:.3e} > {bar:.3e} at {idx} = {a_} "
                           f"(worst of the tensor {worst:.3e} at {at}; torch fp32 on the CPU {r_cpu:.3e})")


def check_stats(ops, case, y, part, info, rows):
    Cn = y.shape[-1]
    yd = y.double().cpu().reshape(-1, Cn)
    mu, var = yd.mean(0), yd.var(0, unbiased=False)
    invstd = 1.0 / torch.sqrt(var + EPS)
    mean_d, invstd_d = ops.bn_finalize(part, info, rows, Cn, EPS, 0.1, None, None)
    e_mu = float((mean_d.double().cpu() - mu).abs().max()) / float(yd.abs().max())
    e_is = float(((invstd_d.double().cpu() - invstd).abs() / invstd).max())
    print(f"forward statistics {T.case_id(case)}: mean {e_mu:.2e} of max|y| (2e-6), invstd {e_is:.2e} (1e-5)")
    assert e_mu <= 2e-6 and e_is <= 1e-5, f"forward statistics {case}: mean {e_mu:.2e} of max|y|, invstd {e_is:.2e}"


# ---- operands and fp64 references -------------------------------------------------------------------------------------------
def fwd_operands(case, hard):
    N, H, W, Ci, Co, k, s, p = case
    g = gen(case, 1)
    if hard:
        x, w = hard_operands((N, Ci, H, W), g, -20, 20, -14), hard_operands((Co, Ci, k, k), g, -8, 8, -6)
    else:
        x, w = torch.randn(N, Ci, H, W, generator=g) + 0.5, torch.randn(Co, Ci, k, k, generator=g) / math.sqrt(k * k * Ci)
    return x, w, torch.randn(Co, generator=g)


def dgrad_operands(case, hard):
    N, H, W, Ci, Co, k, s, p = case
    Ho, Wo = T.out_hw(case)
    g = gen(case, 2)
    if hard:
        return hard_operands((N, Co, Ho, Wo), g, -20, 20, -14), hard_operands((Co, Ci, k, k), g, -8, 8, -6)
    return torch.randn(N, Co, Ho, Wo, generator=g) + 0.5, torch.randn(Co, Ci, k, k, generator=g) / math.sqrt(k * k * Co)


def wgrad_operands(case):
    N, H, W, Ci, Co, k, s, p = case
    Ho, Wo = T.out_hw(case)
    g = gen(case, 3)
    return torch.randn(N, Ci, H, W, generator=g) + 0.5, torch.randn(N, Co, Ho, Wo, generator=g), g


def wgrad_autograd(x, dy, wshape, s, p):
    w0 = torch.zeros(wshape, dtype=x.dtype, requires_grad=True)
    F.conv2d(x, w0, None, s, p).backward(dy)
    return w0.grad


# ---- forward ---------------------------------------------------------------------------------------------------------------
def run_forward(ops, dev, case, route, hard):
    N, H, W, Ci, Co, k, s, p = case
    Ho, Wo = T.out_hw(case)
    K = k * k * Ci
    x, w, b = fwd_operands(case, hard)
    ref = nhwc(F.conv2d(x.double(), w.double(), None, s, p))
    mag = nhwc(F.conv2d(x.double().abs(), w.double().abs(), None, s, p))
    cpu = nhwc(F.conv2d(x, w, None, s, p))
    xd, wd = nhwc(x).to(dev), wcl(w).to(dev)
    sub = pixel_subsets((N, Ho, Wo, Co), T.tile_of(T.FWD, route, case), k)
    expect_plan(case, T.FWD, 0, route)
    if hard:
        check(T.FWD, route, "hard operands", case, ops.conv_fwd(xd, wd, None, s, p), ref, mag, K, cpu, sub)
        return
    check(T.FWD, route, "plain", case, ops.conv_fwd(xd, wd, None, s, p), ref, mag, K, cpu, sub)
    expect_plan(case, T.FWD, T.BIAS, route)
    bd = b.double()
    y = ops.conv_fwd(xd, wd, b.to(dev), s, p)
    check(T.FWD, route, "bias", case, y, ref + bd, mag + bd.abs(), K, cpu + b, sub)
    if route == 4:      # the statistics of the thin-input kernel are formed in the same launch
        expect_plan(case, T.FWD, T.BIAS | T.STATS, route)
        y2, part, info = ops.conv_fwd(xd, wd, b.to(dev), s, p, stats=True)
        assert part.shape == (N * Ho * 4, Co, 2) and info[1] == Wo // 4, f"forward {case}: partials {tuple(part.shape)}, {info}"
        assert torch.equal(y2, y), f"forward {case}: the launch with statistics changes y"
        check_stats(ops, case, y2, part, info, N * Ho * Wo)


@pytest.mark.parametrize("case,route", T.FWD_CASES, ids=ids(T.FWD_CASES))
def test_forward_against_fp64(fp32, dev, case, route):
    run_forward(fp32, dev, case, route, False)


# ---- data gradient -----------------------------------------------------------------------------------------------------------
def run_dgrad(ops, dev, case, route, hard):
    N, H, W, Ci, Co, k, s, p = case
    Ho, Wo = T.out_hw(case)
    K = k * k * Co
    dy, w = dgrad_operands(case, hard)
    opad = (H - ((Ho - 1) * s - 2 * p + k), W - ((Wo - 1) * s - 2 * p + k))
    tr = lambda a, f: nhwc(F.conv_transpose2d(a, f, None, s, p, opad))
    ref, mag, cpu = tr(dy.double(), w.double()), tr(dy.double().abs(), w.double().abs()), tr(dy, w)
    assert ref.shape == (N, H, W, Ci)
    expect_plan(case, T.DGRAD, 0, route)
    dx = ops.conv_dgrad(nhwc(dy).to(dev), wcl(w).to(dev), (N, H, W, Ci), s, p)
    check(T.DGRAD, route, "hard operands" if hard else "plain", case, dx, ref, mag, K, cpu,
          pixel_subsets((N, H, W, Ci), T.tile_of(T.DGRAD, route, case), k))


@pytest.mark.parametrize("case,route", T.DGRAD_CASES, ids=ids(T.DGRAD_CASES))
def test_data_gradient_against_fp64(fp32, dev, case, route):
    run_dgrad(fp32, dev, case, route, False)


@pytest.mark.parametrize("direction,case,route", T.HARD_CASES, ids=[f"{DIRS[c[0]].replace(' ', '-')}-{i}" for i, c in zip(ids([c[1:] for c in T.HARD_CASES]), T.HARD_CASES)])
def test_hard_operands(fp32, dev, direction, case, route):
    """all 24 mantissa bits set, exponents 2^-20 .. 2^20 inside one reduction (the generator of test_gpu_conv3x3_plan_cover.py)"""
    (run_forward if direction == T.FWD else run_dgrad)(fp32, dev, case, route, True)


# ---- weight gradient -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,route,nsplit", T.WGRAD_CASES, ids=ids(T.WGRAD_CASES))
def test_weight_gradient_against_fp64(fp32, dev, case, route, nsplit):
    ops = fp32
    N, H, W, Ci, Co, k, s, p = case
    Ho, Wo = T.out_hw(case)
    K = N * Ho * Wo
    expect_plan(case, T.WGRAD, 0, route, nsplit)
    x, dy, g = wgrad_operands(case)
    ref = phys(wgrad_autograd(x.double(), dy.double(), (Co, Ci, k, k), s, p))
    mag = phys(wgrad_autograd(x.double().abs(), dy.double().abs(), (Co, Ci, k, k), s, p))
    cpu = phys(wgrad_autograd(x, dy, (Co, Ci, k, k), s, p))
    xd, dyd = nhwc(x).to(dev), nhwc(dy).to(dev)
    w_like = wcl(torch.empty(Co, Ci, k, k)).to(dev)
    need = ops.lib().buctd_conv2d_wgrad_workspace(C.byref(T.desc(case)))
    sub = wgrad_subsets(case)

    def run(xs, dys, out=None, accumulate=0):
        ops.workspace(need, dev)[:need].fill_(0xFF)        # a slab element the kernels do not write reads as NaN
        if out is None:
            out = wcl(torch.full((Co, Ci, k, k), float("nan"))).to(dev)
        return ops.conv_wgrad(xs, dys, w_like, s, p, out=out, accumulate=accumulate)

    dw = run(xd, dyd)
    check(T.WGRAD, route, "plain", case, phys(dw), ref, mag, K, cpu, sub, idx="(co, r, s, ci)")
    assert torch.equal(dw, run(xd, dyd)), f"weight gradient {case}: two runs differ"
    base = wcl(torch.randn(Co, Ci, k, k, generator=g))
    out = run(xd, dyd, out=base.to(dev), accumulate=1)
    bs = phys(base).double()
    check(T.WGRAD, route, "accumulate", case, phys(out), ref + bs, torch.maximum(mag, bs.abs()), K, None, sub,
          idx="(co, r, s, ci)", scale=2.0)
    if T.is_loop_case(case, route):
        # the same gradient as the sum of two half-batch calls, each below the workgroup cap: every workgroup one tile / row
        h = N // 2
        for part in ((h,) + case[1:], (N - h,) + case[1:]):
            pl = T.plan(part, T.WGRAD)
            assert pl["route"] == route and pl["nsplit"] < nsplit, f"half batch {part}: {pl}"
        halves = run(xd[:h].contiguous(), dyd[:h].contiguous())
        first = phys(halves).double().cpu()
        halves = run(xd[h:].contiguous(), dyd[h:].contiguous(), out=halves, accumulate=1)
        check(T.WGRAD, route, "against two half-batch calls", case, phys(dw), phys(halves).double().cpu(),
              torch.maximum(mag, first.abs()), K, None, sub, idx="(co, r, s, ci)", scale=2.0)


# ---- guard bands: the C entry points, operands between NaN bands, outputs and workspace between sentinel bands ------------------
def launch_guarded(ops, dev, direction, case, route, on):
    N, H, W, Ci, Co, k, s, p = case
    Ho, Wo = T.out_hw(case)
    lib, ptr = ops.lib(), ops.ptr
    d = T.desc(case)
    b = Bands(dev, on)
    if direction == T.FWD:
        x, w, bias = fwd_operands(case, False)
        xd, wd, bd = b.ro(nhwc(x)), b.ro(phys(w).contiguous()), b.ro(bias)
        y = b.new((N, Ho, Wo, Co), "y")
        part = b.new((N * Ho * 4, Co, 2), "the statistics partials") if route == 4 else None
        expect_plan(case, T.FWD, T.BIAS | (T.STATS if route == 4 else 0), route)
        ops.check(lib.buctd_conv2d_fwd(C.byref(d), ptr(xd), ptr(wd), ptr(bd), None, None, None, 0, ptr(y), ptr(part),
                                       ops.stream_ptr()), "conv2d_fwd")
        res = [y] + ([part] if route == 4 else [])
    elif direction == T.DGRAD:
        dy, w = dgrad_operands(case, False)
        dyd, wd = b.ro(nhwc(dy)), b.ro(phys(w).contiguous())
        dx = b.new((N, H, W, Ci), "dx")
        expect_plan(case, T.DGRAD, 0, route)
        ops.check(lib.buctd_conv2d_dgrad(C.byref(d), ptr(dyd), ptr(wd), None, ptr(dx), None, ops.stream_ptr()), "conv2d_dgrad")
        res = [dx]
    else:
        x, dy, _ = wgrad_operands(case)
        xd, dyd = b.ro(nhwc(x)), b.ro(nhwc(dy))
        need = lib.buctd_conv2d_wgrad_workspace(C.byref(d))
        assert need == T.nsplit_of(case, route) * Co * k * k * Ci * 4
        expect_plan(case, T.WGRAD, 0, route, T.nsplit_of(case, route))
        ws = b.new((need // 4,), "the slab workspace")          # exactly the bytes the library asks for, stale NaNs inside
        dw = b.new((Co, k, k, Ci), "dw")
        ops.check(lib.buctd_conv2d_wgrad(C.byref(d), ptr(xd), ptr(dyd), ptr(dw), 0, ptr(ws), need, ops.stream_ptr()), "conv2d_wgrad")
        res = [dw, ws]
    torch.cuda.synchronize()
    b.check(f"{DIRS[direction]} route {route} {case}")
    return [r.clone() for r in res]


@pytest.mark.parametrize("direction,case,route", T.GUARD_CASES,
                         ids=[f"{DIRS[c[0]].replace(' ', '-')}-{i}" for i, c in zip(ids([c[1:] for c in T.GUARD_CASES]), T.GUARD_CASES)])
def test_between_guard_bands(fp32, dev, direction, case, route):
    """A staging loop that reaches past its operand reads NaN and shows up in the result; a store past y, dx, dw, the
    partials or the slab workspace lands in the sentinel.  Ordinary in-bounds allocations only."""
    plain = launch_guarded(fp32, dev, direction, case, route, False)
    guarded = launch_guarded(fp32, dev, direction, case, route, True)
    for i, (a, g) in enumerate(zip(plain, guarded)):
        what = f"{DIRS[direction]} route {route} {case}: result {i}"
        assert torch.isfinite(g).all(), f"{what} picked up a NaN from beyond an operand, or was not written everywhere"
        assert torch.equal(a, g), f"{what} changes with what lies next to the operands"
