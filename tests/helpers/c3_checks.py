"""What the per-plan and the per-group suites of the 3x3 bf16x6 convolution share (tests/test_gpu_conv3x3_plan_cover.py,
tests/test_gpu_conv3x3_groups.py): the inputs of a case with their fp64 references, and the checkers with their bars.  The
metrics and bars are described in the docstring of tests/test_gpu_conv3x3_plan_cover.py; none is taken from what the kernels
give."""
import ctypes as C
import math

import torch
import torch.nn.functional as F

from tests.helpers import c3_cases as T

HARD = (2, 9, 7, 48, 48)          # the shape of the hard-operands test
CONV_CASES = [(s, False) for s in T.CASES] + [(HARD, True)]
WORST = {}


def _id(c):
    return T.case_id(c[0]) + ("-hard" if c[1] else "")


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2)


def wcl(w):
    return w.contiguous(memory_format=torch.channels_last)


class _Bn:
    """the attributes ops.BnAccInput reads from a BatchNorm module"""

    def __init__(self, Cn, dev, seed=0, eps=1e-5, momentum=0.1):
        g = torch.Generator().manual_seed(Cn + seed)
        self.weight = (1.0 + 0.3 * torch.randn(Cn, generator=g)).to(dev)
        self.bias = (0.2 * torch.randn(Cn, generator=g)).to(dev)
        self.running_mean = torch.zeros(Cn, device=dev)
        self.running_var = torch.ones(Cn, device=dev)
        self.eps, self.momentum, self.track_running_stats = eps, momentum, True



def _note(key, val, base, where):
    if key not in WORST or val > WORST[key][0]:
        WORST[key] = (val, base, where)




def in_fp32(ops, fn):
    ops.set_conv_math("fp32")
    try:
        return fn()
    finally:
        ops.set_conv_math("bf16x6")


def plan(shape, option_set):
    from buctd_amd import _C
    out = (C.c_int * 11)()
    assert _C.lib().buctd_conv3x3_bf16x6_plan(*shape, option_set, out) == 0, f"no plan for {shape}"
    return dict(zip(("MF", "NF", "WM", "WN", "single", "col_major", "kernel", "family", "variant", "BM", "BN"), out))


def hard_operands(shape, g, lo, hi, shift):
    """all 24 mantissa bits set, exponents lo..hi (then scaled by 2^shift - exact), random sign"""
    mant = (torch.randint(0, 2 ** 23, shape, generator=g) | 1).float() / 2 ** 23 + 1.0
    v = mant * torch.exp2(torch.randint(lo, hi + 1, shape, generator=g).float() + shift)
    return v * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)


class Inputs:
    """the float inputs of one case (NCHW on the CPU) and, on demand, the fp64 references built from them"""

    def __init__(self, shape, hard):
        N, H, W, Ci, Co = shape
        self.shape, self.hard = shape, hard
        g = torch.Generator().manual_seed(sum(shape) * 31 + Ci)
        if hard:
            # 2^-20..2^20 inside one reduction, moved down by 2^-14 so that the sums of squares of the outputs stay inside
            # the range of the statistics accumulator (bn_acc.h: |sum| < 2^46 per workgroup)
            self.x = hard_operands((N, Ci, H, W), g, -20, 20, -14)
            self.w = hard_operands((Co, Ci, 3, 3), g, -8, 8, -6)
            self.wb = hard_operands((Ci, Co, 3, 3), g, -8, 8, -6)
            self.res = hard_operands((N, Co, H, W), g, -20, 20, -14)
        else:
            self.x = torch.randn(N, Ci, H, W, generator=g) + 0.5
            self.w = torch.randn(Co, Ci, 3, 3, generator=g) / math.sqrt(9 * Ci)
            self.wb = torch.randn(Ci, Co, 3, 3, generator=g) / math.sqrt(9 * Ci)     # forward Co -> Ci: its data gradient is Ci -> Co
            self.res = torch.randn(N, Co, H, W, generator=g)
        self.bias = torch.randn(Co, generator=g)
        self.scale, self.shift = torch.rand(Co, generator=g) + 0.5, torch.randn(Co, generator=g)
        self.zb = torch.randn(N, H, W, Co, generator=g) * 1.7 + 0.3                   # the z of the BatchNorm whose backward consumes dx
        self.r2 = torch.randn(N, H, W, Co, generator=g)
        self.memo = {}

    def get(self, key, fn):
        if key not in self.memo:
            self.memo[key] = fn()
        return self.memo[key]

    def fwd(self):      # conv(x, w) and conv(|x|, |w|), NHWC double
        return self.get("fwd", lambda: (nhwc(F.conv2d(self.x.double(), self.w.double(), None, 1, 1)),
                                        nhwc(F.conv2d(self.x.double().abs(), self.w.double().abs(), None, 1, 1))))

    def dgrad(self):    # the data gradient of the forward convolution wb (Co -> Ci) at dy = x
        return self.get("dgrad", lambda: (nhwc(F.conv_transpose2d(self.x.double(), self.wb.double(), None, 1, 1)),
                                          nhwc(F.conv_transpose2d(self.x.double().abs(), self.wb.double().abs(), None, 1, 1))))


_last = {}


def inputs(case):
    if _last.get("case") != case:
        _last.clear()
        _last.update(case=case, inp=Inputs(*case))
    return _last["inp"]


def subsets(shape, pl):
    """boolean masks [N, H, W, Co]-broadcastable: whole tensor, last position tile, last column tile, image borders"""
    N, H, W, Ci, Co = shape
    SW, IB = W + 1, (H + 1) * (W + 1)
    n, y, x = torch.meshgrid(torch.arange(N), torch.arange(H), torch.arange(W), indexing="ij")
    p = n * IB + (y + 1) * SW + (x + 1)                         # the padded flattened position of a pixel (c3_common.h)
    last_tile = (p // pl["BM"] == int(p.max()) // pl["BM"])[..., None].expand(N, H, W, Co)
    last_col = (torch.arange(Co) >= Co - pl["BN"]).expand(N, H, W, Co)
    border = ((y == 0) | (y == H - 1) | (x == 0) | (x == W - 1))[..., None].expand(N, H, W, Co)
    return {"whole tensor": None, "last position tile": last_tile, "last column tile": last_col, "border pixels": border}


def check_conv(name, opt, case, got, got32, ref, mag):
    """got / got32: the bf16x6 and the exact-fp32 kernel's output (NHWC, device); ref / mag: fp64 value and sum of |terms|"""
    shape = case[0]
    pl = plan(shape, T.OPTION_SETS[opt])
    mag = mag.clamp_min(1e-300)
    r = (got.double().cpu() - ref).abs() / mag
    r32 = float(((got32.double().cpu() - ref).abs() / mag).max())
    bar = min(2e-6, 3 * r32 + 2e-7)
    worst = float(r.max())
    at = tuple(int(v) for v in torch.unravel_index(r.argmax(), r.shape))
    print(f"{opt} {name} {_id(case)}: error / sum|terms| bf16x6 {worst:.3e}, exact-fp32 kernel {r32:.3e} (bar {bar:.3e}); "
          f"kernel {pl['kernel']} MF {pl['MF']} NF {pl['NF']} {pl['WM']}x{pl['WN']}")
    _note(f"{opt}: conv", worst, r32, _id(case))
    assert torch.isfinite(got).all(), f"{opt} {name} {shape}: non-finite output"
    for where, m in subsets(shape, pl).items():
        rr = r if m is None else torch.where(m, r, torch.zeros((), dtype=r.dtype))
        w_ = float(rr.max())
        a_ = tuple(int(v) for v in torch.unravel_index(rr.argmax(), rr.shape))
        assert w_ <= bar, (f"{opt} {name} {shape} [{where}]: error / sum|terms| {w_:.3e} > {bar:.3e} at (n, h, w, c) = {a_} "
                           f"(fp32 kernel {r32:.3e}; worst of the tensor {worst:.3e} at {at}; plan {pl})")


def check_stats(name, opt, case, z, bnin, bn, y=None, res=None, relu=True):
    """forward statistics decoded from an accumulator against fp64 statistics of the device's own z"""
    Cn = z.shape[-1]
    zd = z.double().cpu().reshape(-1, Cn)
    rows = zd.shape[0]
    mu, var = zd.mean(0), zd.var(0, unbiased=False)
    invstd = 1.0 / torch.sqrt(var + bn.eps)
    e_mu = float(((bnin.mean.double().cpu() - mu).abs() / mu.abs().clamp_min(1.0)).max())
    e_is = float(((bnin.invstd.double().cpu() - invstd).abs() / invstd).max())
    rm = bn.momentum * mu
    rv = (1 - bn.momentum) + bn.momentum * var * rows / (rows - 1)
    e_rm = float(((bn.running_mean.double().cpu() - rm).abs() / rm.abs().clamp_min(1.0)).max())
    e_rv = float(((bn.running_var.double().cpu() - rv).abs() / rv).max())
    print(f"{opt} {name} {_id(case)}: mean {e_mu:.2e} (2e-6), invstd {e_is:.2e} (3e-7), running_mean {e_rm:.2e} (1e-6), "
          f"running_var {e_rv:.2e} (1e-6)")
    _note(f"{opt}: invstd", e_is, 3e-7, _id(case))
    assert e_mu <= 2e-6 and e_is <= 3e-7 and e_rm <= 1e-6 and e_rv <= 1e-6, f"{opt} {name} {case[0]}"
    if y is not None:
        yr = (zd - mu) * invstd * bn.weight.double().cpu() + bn.bias.double().cpu()
        if res is not None:
            yr = yr + res.double().cpu().reshape(-1, Cn)
        if relu:
            yr = torch.relu(yr)
        e = (y.double().cpu().reshape(-1, Cn) - yr).abs() / yr.abs().clamp_min(1.0)
        assert float(e.max()) <= 2e-5, f"{opt} {name} {case[0]}: applied output off by {float(e.max()):.2e} at row, channel " \
                                       f"{tuple(int(v) for v in torch.unravel_index(e.argmax(), e.shape))}"


def bn_backward_reference(g, z, res, gamma, beta, m, dtype):
    """autograd of BatchNorm (train mode) (+ residual) + ReLU with the ReLU mask m given: -> dz, dgamma (= s2), dbeta (= s1)"""
    Cn = z.shape[-1]
    zz = z.to(dtype).reshape(-1, Cn).requires_grad_(True)
    ga, be = gamma.to(dtype).requires_grad_(True), beta.to(dtype).requires_grad_(True)
    mu, var = zz.mean(0), zz.var(0, unbiased=False)
    out = (zz - mu) / torch.sqrt(var + 1e-5) * ga + be
    if res is not None:
        out = out + res.to(dtype).reshape(-1, Cn)
    (out * m.to(dtype).reshape(-1, Cn)).backward(g.to(dtype).reshape(-1, Cn))
    return zz.grad.reshape(z.shape), ga.grad, be.grad


def check_bn_backward(opt, case, g_dev, dz, dgamma, dbeta, z, res, gamma, beta, m):
    g = g_dev.cpu()
    ref = bn_backward_reference(g, z, res, gamma, beta, m, torch.float64)
    cpu = bn_backward_reference(g, z, res, gamma, beta, m, torch.float32)
    for name, got, r64, r32 in zip(("dz", "s2 = sum m g zhat (dgamma)", "s1 = sum m g (dbeta)"), (dz, dgamma, dbeta), ref, cpu):
        top = float(r64.abs().max())
        e = (got.double().cpu() - r64).abs() / top
        e_cpu = float((r32.double() - r64).abs().max()) / top
        bar = max(5e-6, 4 * e_cpu)
        at = tuple(int(v) for v in torch.unravel_index(e.argmax(), e.shape))
        print(f"{opt} {name} {_id(case)}: rel. error vs fp64 {float(e.max()):.3e}, fp32 on the CPU {e_cpu:.3e} (bar {bar:.3e})")
        _note(f"{opt}: {name.split(' ')[0]}", float(e.max()), e_cpu, _id(case))
        assert float(e.max()) <= bar, f"{opt} {name} {case[0]}: {float(e.max()):.3e} > {bar:.3e} at {at} (fp32 CPU {e_cpu:.3e})"


def bn_params(inp, dev):
    """the BatchNorm behind the data gradient: float batch statistics of zb (what its forward left), gamma, beta"""
    Co = inp.shape[4]
    zd = inp.zb.double().reshape(-1, Co)
    mean = zd.mean(0).float()
    invstd = (1.0 / torch.sqrt(zd.var(0, unbiased=False) + 1e-5)).float()
    bn = _Bn(Co, dev, seed=3)
    return mean, invstd, bn.weight.cpu(), bn.bias.cpu()


def bnstat_acc(ops, shape, x, wb, residual, dx, bn_z, bn_y, mean, invstd, gamma, beta):
    """buctd_conv3x3_bf16x6_bnstat_acc as block.hip calls it, then the consumer of the accumulator (buctd_bn_bwd_acc with
    acc_ready = 1): -> dz, dgamma, dbeta"""
    N, H, W, Ci, Co = shape
    lib, ptr = ops.lib(), ops.ptr
    dev = x.device
    acc = ops.AccRef(Co, dev)
    wp = ops._conv3x3_prepared(wb, 1)
    ops.check(lib.buctd_conv3x3_bf16x6_bnstat_acc(N, H, W, Ci, Co, ptr(x), ptr(wp), ptr(residual), ptr(dx), ptr(bn_z), ptr(bn_y),
                                                  ptr(mean), ptr(invstd), ptr(gamma), ptr(beta), C.c_void_p(acc.ptr),
                                                  ops.stream_ptr()), "conv3x3_bf16x6_bnstat_acc")
    dz = torch.empty_like(bn_z)
    dgamma, dbeta = torch.empty(Co, device=dev), torch.empty(Co, device=dev)
    ops.check(lib.buctd_bn_bwd_acc(ptr(dx), ptr(bn_y), ptr(bn_z), ptr(mean), ptr(invstd), ptr(gamma), ptr(beta), 1, N * H * W, Co,
                                   ptr(dz), None, ptr(dgamma), ptr(dbeta), 0, C.c_void_p(acc.ptr), 1, ops.stream_ptr()),
              "bn_bwd_acc")
    return dz, dgamma, dbeta


def rebuilt_mask(ops, inp, mean, invstd, gamma, beta, dev):
    """The ReLU mask (z - mean) (invstd gamma) + beta > 0 in fp64; where the value is within fp32 rounding of zero the sign is
    undecided and the device's own forward (bn_apply, whose expression the kernel documents it rebuilds) decides."""
    v = (inp.zb.double() - mean.double()) * (invstd.double() * gamma.double()) + beta.double()
    band = v.abs() <= 4e-7 * ((inp.zb.double() - mean.double()).abs() * (invstd.double() * gamma.double()).abs() + beta.double().abs())
    yd = ops.bn_apply(inp.zb.to(dev), mean.to(dev), invstd.to(dev), gamma.to(dev), beta.to(dev), None, True).cpu()
    return torch.where(band, yd > 0, v > 0)

def check_wgrad(name, case, got, got32, ref, mag):
    mag = mag.clamp_min(1e-300)
    r = (got.double().cpu() - ref).abs() / mag
    r32 = float(((got32.double().cpu() - ref).abs() / mag).max())
    bar = min(2e-6, 3 * r32 + 2e-7)
    at = tuple(int(v) for v in torch.unravel_index(r.argmax(), r.shape))
    print(f"wgrad {name} {_id(case)}: error / sum|terms| bf16x6 {float(r.max()):.3e}, exact-fp32 kernel {r32:.3e} (bar {bar:.3e})")
    _note("wgrad", float(r.max()), r32, _id(case))
    assert torch.isfinite(got).all() and float(r.max()) <= bar, \
        f"wgrad {name} {case[0]}: {float(r.max()):.3e} > {bar:.3e} at (co, ci, r, s) = {at} (fp32 kernel {r32:.3e})"


def wgrad_ref(x, dy, shape):
    """x, dy: NCHW double"""
    N, H, W, Ci, Co = shape
    return torch.nn.grad.conv2d_weight(x, (Co, Ci, 3, 3), dy, stride=1, padding=1)
