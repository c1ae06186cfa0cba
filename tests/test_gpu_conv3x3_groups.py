"""The group launches of the 3x3 bf16x6 convolution (buctd_conv3x3_bf16x6_group / _group_eval, buctd_conv3x3_wgrad_bf16x6_group):
every group of tests/helpers/c3_group_cases.py x every option set, through the C entry points.  The host-only closure test
(test_conv3x3_group_cover.py) proves that the groups reach every kernel variant as a member of a multi-member launch.

Per group and option set:
  guard bands       every output of every member (y, statistics accumulator, mean_out / invstd_out / running statistics,
                    BatchNorm-backward accumulator) lies between sentinel bands, every operand between NaN bands;
  single launches   every member's outputs equal, bit for bit, its own buctd_conv3x3_bf16x6_acc / _bnstat_acc /
                    buctd_conv3x3_bf16x6 launch on the same operands (the library's contract; accumulators are integers);
  fp64              independently of that, the checkers and bars of test_gpu_conv3x3_plan_cover.py (tests/helpers/c3_checks.py)
                    on each member's GROUP result: whole tensor, last position tile, last column tile, borders;
  reproducibility   a second run of the group gives the same bits.
Weight-gradient groups: check_wgrad's metric and bar against fp64 (x_bn members: the gradient with respect to the normalised
and ReLU-ed input; accumulate members: reference + previous contents), guard bands around every dw and every workspace, the
member's single launch to 5e-6 of the largest element (another split count, another summation order), run-to-run bits, and the
refusals (workspace one byte short, mixed chunk widths) with untouched bands.

Measured on an MI355X: worst figure per option set over all groups and members, next to the baseline it was judged against (the
exact-fp32 kernel's ratio for the convolution outputs, the fp32 CPU evaluation for the BatchNorm-backward quantities):
  option set    conv ratio / fp32 kernel   invstd (bar 3e-7)   s1 / fp32 CPU        s2 / fp32 CPU        dz / fp32 CPU
  general       2.81e-07 / 3.24e-07
  STATS         3.22e-07 / 3.21e-07        1.2e-07
  STATS|IN_BN   4.07e-07 / 3.48e-07        9.7e-08
  RES           3.03e-07 / 2.58e-07
  BS_REBUILD    3.11e-07 / 2.81e-07                            4.2e-08 / 7.7e-08    8.9e-08 / 8.4e-08    1.6e-07 / 1.1e-07
  RES|BS_Y      3.03e-07 / 2.58e-07                            8.2e-08 / 9.8e-08    1.1e-07 / 8.9e-08    1.4e-07 / 1.0e-07
  wgrad         2.41e-07 / 1.71e-07
Every bit-for-bit comparison held; no defect was found in a group kernel.  Wall time of the module: 10.7 s (51 tests; the
slowest, f1-general, 1.3 s)."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import c3_cases as T
from tests.helpers import c3_group_cases as G
from tests.helpers.c3_checks import (WORST, Inputs, _Bn, bn_params, check_bn_backward, check_conv, check_stats, check_wgrad,
                                     in_fp32, nchw, nhwc, rebuilt_mask, wcl, wgrad_ref)
from tests.helpers.guard_bands import SENTINEL, banded16, untouched

pytestmark = pytest.mark.gpu

PAD = 4096          # elements on either side of an output: a multiple of 256 bytes for every type used here
ISENT = -12345


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


_inputs = {}


def inputs(shape):
    """the inputs and (memoised) fp64 references of a member, shared by the option sets and the groups that hold it"""
    if shape not in _inputs:
        _inputs[shape] = Inputs(shape, False)
    return _inputs[shape]


class Place:
    """on=True: read-only operands between NaN bands, outputs between sentinel bands; on=False: plain tensors"""

    def __init__(self, dev, on):
        self.dev, self.on, self.keep, self.outs = dev, on, [], []

    def ro(self, t):
        if t is None:
            return None
        if not self.on:
            t = t.to(self.dev).contiguous()
            self.keep.append(t)
            return t
        view, big, _ = banded16(t.contiguous(), self.dev)
        self.keep.append(big)
        return view

    def out(self, init, name):
        if not self.on:
            t = init.to(self.dev).clone().contiguous()
            self.keep.append(t)
            return t
        fill = SENTINEL if init.dtype.is_floating_point else ISENT
        big = torch.full((2 * PAD + init.numel(),), fill, dtype=init.dtype, device=self.dev)
        view = big[PAD:PAD + init.numel()].view(init.shape)
        view.copy_(init)
        assert view.data_ptr() % 256 == 0
        self.outs.append((big, init.numel(), fill, name))
        return view

    def new(self, shape, name):
        return self.out(torch.full(tuple(shape), float("nan")), name)

    def acc(self, ops, Cn, name):
        """a zeroed statistics accumulator (csrc/bn_acc.h) of Cn channels"""
        return self.out(torch.zeros(ops.acc_bytes(Cn) // 8, dtype=torch.int64), name)

    def check(self, what):
        for big, n, fill, name in self.outs:
            assert untouched(big, PAD, n, fill), f"{what}: the launch wrote outside {name}"


class AccPtr:
    """what ops.BnAccInput reads of an accumulator"""

    def __init__(self, t, Cn):
        self.t, self.Cn, self.ptr = t, Cn, t.data_ptr()


def p(t):
    return None if t is None else t.data_ptr()


# ---- one member under one option set: operands, outputs, the group item, its single launch ------------------------------------
class Member:
    def __init__(self, ops, dev, shape, opt, pl, tag, producer):
        """pl: a Place; producer: (z1, acc1, bn1, w0) of the STATS|IN_BN input, shared by every run of the member"""
        self.ops, self.dev, self.shape, self.opt, self.tag = ops, dev, shape, opt, tag
        N, H, W, Ci, Co = shape
        inp = self.inp = inputs(shape)
        fwd = opt in ("general", "STATS", "STATS|IN_BN")
        self.w = wcl(inp.w if fwd else inp.wb).to(dev)
        self.wp = ops._conv3x3_prepared(self.w, 0 if fwd else 1)
        self.x = pl.ro(nhwc(inp.x)) if opt != "STATS|IN_BN" else pl.ro(producer[0])
        self.y = pl.new((N, H, W, Co), f"y of {tag}")
        self.out = {"y": self.y}
        if opt == "general":
            self.scale, self.shift, self.res = pl.ro(inp.scale), pl.ro(inp.shift), pl.ro(nhwc(inp.res))
        if opt in ("STATS", "STATS|IN_BN"):
            self.acc = self.out["stats_acc"] = pl.acc(ops, Co, f"stats_acc of {tag}")
        if opt == "STATS|IN_BN":
            z1, acc1, bn1, _ = producer
            self.bn1 = _Bn(Ci, dev, seed=1)
            self.gamma, self.beta = pl.ro(self.bn1.weight), pl.ro(self.bn1.bias)
            for k in ("mean_out", "invstd_out"):
                self.out[k] = pl.new((Ci,), f"{k} of {tag}")
            self.out["running_mean"] = pl.out(torch.zeros(Ci), f"running_mean of {tag}")
            self.out["running_var"] = pl.out(torch.ones(Ci), f"running_var of {tag}")
            st = self.st = ops._C.BnAccIn()
            st.acc, st.rows, st.eps, st.momentum = acc1.ptr, N * H * W, self.bn1.eps, self.bn1.momentum
            st.mean_out, st.invstd_out = p(self.out["mean_out"]), p(self.out["invstd_out"])
            st.running_mean, st.running_var = p(self.out["running_mean"]), p(self.out["running_var"])
        if opt in ("RES", "RES|BS_Y"):
            self.res = pl.ro(nhwc(inp.res))
        if opt in ("BS_REBUILD", "RES|BS_Y"):
            mean, invstd, gamma, beta = self.bnp = bn_params(inp, dev)
            self.zb, self.mean, self.invstd, self.gamma = pl.ro(inp.zb), pl.ro(mean), pl.ro(invstd), pl.ro(gamma)
            self.beta = pl.ro(beta) if opt == "BS_REBUILD" else None
            self.yb = None
            if opt == "RES|BS_Y":
                self.yb_cpu = torch.relu(((inp.zb.double() - mean.double()) * (invstd.double() * gamma.double()) + beta.double()
                                          + inp.r2.double())).float()
                self.yb = pl.ro(self.yb_cpu)
            self.bacc = self.out["bn_acc"] = pl.acc(ops, Co, f"bn_acc of {tag}")

    def fill(self, it):
        """it: _C.C3Conv, or _C.C3ConvEval for the eval entry point"""
        it.N, it.H, it.W, it.Ci, it.Co = self.shape
        it.x, it.wprep, it.y = p(self.x), p(self.wp), p(self.y)
        o = self.opt
        if o == "general":
            it.scale, it.shift, it.residual, it.relu = p(self.scale), p(self.shift), p(self.res), 1
        if o in ("STATS", "STATS|IN_BN"):
            it.stats_acc = p(self.acc)
        if o == "STATS|IN_BN":
            it.in_bn = C.pointer(self.st)
            it.in_gamma, it.in_beta, it.in_relu = p(self.gamma), p(self.beta), 1
        if o in ("RES", "RES|BS_Y"):
            it.residual = p(self.res)
        if o in ("BS_REBUILD", "RES|BS_Y"):
            it.bn_z, it.bn_y, it.bn_mean, it.bn_invstd = p(self.zb), p(self.yb), p(self.mean), p(self.invstd)
            it.bn_gamma, it.bn_beta, it.bn_acc = p(self.gamma), p(self.beta), p(self.bacc)

    def single(self):
        """the member's own launch, as the library documents it"""
        ops, lib, o = self.ops, self.ops.lib(), self.opt
        s, st = self.shape, ops.stream_ptr()
        if o == "general":
            rc = lib.buctd_conv3x3_bf16x6(*s, p(self.x), p(self.wp), None, p(self.scale), p(self.shift), p(self.res), 1, p(self.y),
                                          None, None, st)
        elif o == "STATS":
            rc = lib.buctd_conv3x3_bf16x6_acc(*s, p(self.x), p(self.wp), None, 0, p(self.y), p(self.acc), None, None, None, 0, st)
        elif o == "STATS|IN_BN":
            rc = lib.buctd_conv3x3_bf16x6_acc(*s, p(self.x), p(self.wp), None, 0, p(self.y), p(self.acc), C.byref(self.st),
                                              p(self.gamma), p(self.beta), 1, st)
        elif o == "RES":
            rc = lib.buctd_conv3x3_bf16x6(*s, p(self.x), p(self.wp), None, None, None, p(self.res), 0, p(self.y), None, None, st)
        else:
            rc = lib.buctd_conv3x3_bf16x6_bnstat_acc(*s, p(self.x), p(self.wp), p(self.res) if o == "RES|BS_Y" else None, p(self.y),
                                                     p(self.zb), p(self.yb), p(self.mean), p(self.invstd), p(self.gamma),
                                                     p(self.beta), p(self.bacc), st)
        ops.check(rc, f"single launch of {self.tag}")

    def snapshot(self):
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in self.out.items()}


def producer_of(ops, dev, shape):
    """STATS|IN_BN: the convolution whose raw output z1 and statistics accumulator are the member's input"""
    N, H, W, Ci, Co = shape
    inp = inputs(shape)
    g = torch.Generator().manual_seed(Ci + 11)
    w0 = torch.randn(Ci, Ci, 3, 3, generator=g) / math.sqrt(9 * Ci)
    z1, acc1, info = ops.conv_fwd(nhwc(inp.x).to(dev), wcl(w0).to(dev), None, 1, 1, stats="acc")
    assert info[0] == "acc"
    return z1, acc1, None, w0


def launch_group(ops, opt, members):
    from buctd_amd import _C
    n = len(members)
    items = ((_C.C3ConvEval if opt == "general" else _C.C3Conv) * n)()
    for it, m in zip(items, members):
        m.fill(it)
    fn = ops.lib().buctd_conv3x3_bf16x6_group_eval if opt == "general" else ops.lib().buctd_conv3x3_bf16x6_group
    return fn(n, items, ops.stream_ptr())


def bn_bwd_from_acc(ops, m, dx, bacc):
    """the consumer of the BatchNorm-backward accumulator (buctd_bn_bwd_acc, acc_ready = 1) -> dz, dgamma, dbeta"""
    N, H, W, Ci, Co = m.shape
    dz = torch.empty((N, H, W, Co), device=m.dev)
    dgamma, dbeta = torch.empty(Co, device=m.dev), torch.empty(Co, device=m.dev)
    acc = bacc.clone()
    ops.check(ops.lib().buctd_bn_bwd_acc(p(dx), p(m.yb), p(m.zb), p(m.mean), p(m.invstd), p(m.gamma), p(m.beta), 1, N * H * W, Co,
                                         p(dz), None, p(dgamma), p(dbeta), 0, p(acc), 1, ops.stream_ptr()), "bn_bwd_acc")
    return dz, dgamma, dbeta


def check_member_fp64(ops, dev, m, got, gid):
    """the member's GROUP result against fp64, with the checkers and bars of the per-plan module"""
    opt, inp, shape = m.opt, m.inp, m.shape
    N, H, W, Ci, Co = shape
    case = (shape, False)
    name = f"[group {gid}, member {m.tag}]"
    xd = nhwc(inp.x).to(dev)
    if opt == "general":
        ref, mag = inp.fwd()
        rd = nhwc(inp.res).double()
        sc, sh, resd = inp.scale.to(dev), inp.shift.to(dev), nhwc(inp.res).to(dev)
        y32 = inp.get("ev32", lambda: in_fp32(ops, lambda: ops.conv_fwd(xd, m.w, None, 1, 1, scale=sc, shift=sh, residual=resd,
                                                                        relu=True)).cpu())
        check_conv(name + " scale/shift/residual/relu", opt, case, got["y"], y32,
                   torch.relu(ref * inp.scale.double() + inp.shift.double() + rd),
                   mag * inp.scale.double().abs() + inp.shift.double().abs() + rd.abs())
    elif opt == "STATS":
        ref, mag = inp.fwd()
        z32 = inp.get("z32", lambda: in_fp32(ops, lambda: ops.conv_fwd(xd, m.w, None, 1, 1)).cpu())
        check_conv(name + " z", opt, case, got["y"], z32, ref, mag)
        bn = _Bn(Co, dev)
        bnin = ops.BnAccInput(AccPtr(got["stats_acc"], Co), N * H * W, bn, True)
        resd = nhwc(inp.res).to(dev)
        y = ops.bn_apply_acc(got["y"], bnin, resd, True)
        check_stats(name + " statistics", opt, case, got["y"], bnin, bn, y, resd)
    elif opt == "STATS|IN_BN":
        z1 = m.x
        bn1 = m.bn1
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
        z32 = in_fp32(ops, lambda: ops.conv_fwd(y1f, m.w, None, 1, 1))
        check_conv(name + " z of conv(relu(bn(z1)))", opt, case, got["y"], z32, ref, mag)

        class St:
            pass
        st, bnr = St(), St()
        st.mean, st.invstd = got["mean_out"], got["invstd_out"]
        bnr.eps, bnr.momentum, bnr.running_mean, bnr.running_var = bn1.eps, bn1.momentum, got["running_mean"], got["running_var"]
        check_stats(name + " the producer's statistics (mean_out, invstd_out, running)", opt, case, z1, st, bnr)
        bn2 = _Bn(Co, dev, seed=2)
        bnin2 = ops.BnAccInput(AccPtr(got["stats_acc"], Co), N * H * W, bn2, True)
        y = ops.bn_apply_acc(got["y"], bnin2, None, True)
        check_stats(name + " its own statistics", opt, case, got["y"], bnin2, bn2, y)
    else:
        dref, dmag = inp.dgrad()
        dx32 = inp.get("dx32", lambda: in_fp32(ops, lambda: ops.conv_dgrad(xd, m.w, (N, H, W, Co), 1, 1)).cpu())
        if opt in ("RES", "RES|BS_Y"):
            rd = nhwc(inp.res)
            dref, dmag, dx32 = dref + rd.double(), dmag + rd.double().abs(), dx32 + rd
        check_conv(name + " dx", opt, case, got["y"], dx32, dref, dmag)
        if opt != "RES":
            mean, invstd, gamma, beta = m.bnp
            if opt == "RES|BS_Y":
                mask, res_bn = m.yb_cpu > 0, inp.r2
            else:
                mask, res_bn = inp.get("mask", lambda: rebuilt_mask(ops, inp, mean, invstd, gamma, beta, dev)), None
            dz, dgamma, dbeta = bn_bwd_from_acc(ops, m, got["y"], got["bn_acc"])
            check_bn_backward(opt, case, got["y"], dz, dgamma, dbeta, inp.zb, res_bn, gamma, beta, mask)


def first_difference(a, b):
    d = (a != b).reshape(a.shape)
    idx = tuple(int(v) for v in torch.nonzero(d)[0])
    return idx, a[idx].item(), b[idx].item(), int(d.sum())


def run_conv_group(ops, dev, gname, shapes, opt, expect_one_kernel):
    gid = G.group_id(gname, opt)
    plan = G.group_plan(shapes, T.OPTION_SETS[opt])
    assert plan["one_kernel"] == expect_one_kernel, f"{gid}: {plan}"
    producers = [producer_of(ops, dev, s) if opt == "STATS|IN_BN" else None for s in shapes]
    tags = [f"{k} {T.case_id(s)}" for k, s in enumerate(shapes)]
    runs = []
    for rep in range(2):
        pl = Place(dev, True)
        members = [Member(ops, dev, s, opt, pl, tag, pr) for s, tag, pr in zip(shapes, tags, producers)]
        ops.check(launch_group(ops, opt, members), f"group {gid}")
        torch.cuda.synchronize()
        pl.check(f"group {gid}")
        runs.append([m.snapshot() for m in members])
    # the members' own launches, on plain tensors
    pl1 = Place(dev, False)
    singles = [Member(ops, dev, s, opt, pl1, tag, pr) for s, tag, pr in zip(shapes, tags, producers)]
    for m in singles:
        m.single()
    alone = [m.snapshot() for m in singles]
    for m, got, again, one in zip(members, runs[0], runs[1], alone):
        for k in got:
            assert got[k].is_floating_point() is False or torch.isfinite(got[k]).all(), \
                f"group {gid}, member {m.tag}: {k} is not finite (a NaN from beyond an operand, or an element never written)"
            if not torch.equal(got[k], one[k]):
                idx, a, b, cnt = first_difference(got[k], one[k])
                raise AssertionError(f"group {gid}, member {m.tag}, option set {opt}: {k} differs from the member's own launch in "
                                     f"{cnt} elements, first at {idx}: group {a!r}, single {b!r}; plan {plan}")
            assert torch.equal(got[k], again[k]), f"group {gid}, member {m.tag}: {k} is not run-to-run reproducible"
    for m, got in zip(members, runs[0]):
        check_member_fp64(ops, dev, m, got, gid)


CONV_RUNS = [(name, opt) for opt in T.OPTION_SETS for name in G.conv_groups(opt)]


@pytest.mark.parametrize("name,opt", CONV_RUNS, ids=[G.group_id(n, o) for n, o in CONV_RUNS])
def test_group_x_option_set(x6, dev, name, opt):
    run_conv_group(x6, dev, name, G.conv_groups(opt)[name], opt, True)


@pytest.mark.parametrize("opt", [o for o in T.OPTION_SETS if o != "general"])
def test_group_without_a_common_family_runs_one_launch_per_member(x6, dev, opt):
    run_conv_group(x6, dev, "no-family", G.NO_FAMILY_GROUP, opt, False)


def test_in_bn_member_without_an_accumulator_is_refused(x6, dev):
    from buctd_amd import _C
    ops = x6
    shapes = G.TRAIN_GROUPS["f1-twins"]
    pl = Place(dev, True)
    producers = [producer_of(ops, dev, s) for s in shapes]
    members = [Member(ops, dev, s, "STATS|IN_BN", pl, f"{k}", pr) for k, (s, pr) in enumerate(zip(shapes, producers))]
    members[1].st.acc = None
    rc = launch_group(ops, "STATS|IN_BN", members)
    torch.cuda.synchronize()
    assert rc != 0
    with pytest.raises(_C.BuctdHipError, match="in_bn without an accumulator"):
        ops.check(rc, "group")
    pl.check("refused group")
    for m in members:
        assert torch.isnan(m.y).all() and int(m.acc.abs().sum()) == 0, "a refused call must not launch anything"


# ---- weight gradient ------------------------------------------------------------------------------------------------------
class WgMember:
    def __init__(self, ops, dev, member, n, pl, tag):
        shape, self.accumulate, self.x_bn = member
        self.shape, self.tag, self.dev = shape, tag, dev
        N, H, W, Ci, Co = shape
        g = torch.Generator().manual_seed(sum(shape) * 17 + Co)
        self.xc, self.dyc = torch.randn(N, Ci, H, W, generator=g) + 0.5, torch.randn(N, Co, H, W, generator=g)
        self.prev = torch.randn(Co, 3, 3, Ci, generator=g)                # physical [Co][3][3][Ci]
        self.x, self.dy = pl.ro(nhwc(self.xc)), pl.ro(nhwc(self.dyc))
        self.dw = pl.out(self.prev if self.accumulate else torch.full((Co, 3, 3, Ci), float("nan")), f"dw of {tag}")
        self.need = ops.lib().buctd_conv3x3_wgrad_bf16x6_group_workspace(n, *shape)
        assert self.need > 0 and self.need % 4 == 0
        self.ws = pl.out(torch.full((self.need // 4,), float("nan")), f"workspace of {tag}")
        if self.x_bn:
            zd = self.xc.double()
            self.bn = _Bn(Ci, dev, seed=4)
            self.mean_c = zd.mean((0, 2, 3)).float()
            self.invstd_c = (1.0 / torch.sqrt(zd.var((0, 2, 3), unbiased=False) + 1e-5)).float()
            self.mean, self.invstd = pl.ro(self.mean_c), pl.ro(self.invstd_c)
            self.gamma, self.beta = pl.ro(self.bn.weight), pl.ro(self.bn.bias)

    def fill(self, it, short=0):
        it.N, it.H, it.W, it.Ci, it.Co = self.shape
        it.x, it.dy, it.dw, it.accumulate = p(self.x), p(self.dy), p(self.dw), self.accumulate
        it.workspace, it.workspace_bytes = p(self.ws), self.need - short
        if self.x_bn:
            it.x_mean, it.x_invstd, it.x_gamma, it.x_beta, it.x_relu = p(self.mean), p(self.invstd), p(self.gamma), p(self.beta), 1

    def reference(self):
        """fp64 gradient and sum of |terms| as [Co][Ci][3][3], and the operand the exact-fp32 kernel gets for x"""
        x, dy = self.xc.double(), self.dyc.double()
        xa = x.abs()
        xf = nhwc(self.xc)
        if self.x_bn:
            v = lambda t: t.double().cpu().view(1, -1, 1, 1)
            a = (x - v(self.mean_c)) * (v(self.invstd_c) * v(self.bn.weight))
            x = torch.relu(a + v(self.bn.bias))
            xa = torch.where(x > 0, a.abs() + v(self.bn.bias).abs(), torch.zeros((), dtype=torch.float64))
            xf = nhwc(x.float())
        ref, mag = wgrad_ref(x, dy, self.shape), wgrad_ref(xa, dy.abs(), self.shape)
        if self.accumulate:
            prev = self.prev.permute(0, 3, 1, 2).double()
            ref, mag = ref + prev, mag + prev.abs()
        return ref, mag, xf


def launch_wgrad(ops, members, short=None):
    from buctd_amd import _C
    items = (_C.Wg3Conv * len(members))()
    for k, (it, m) in enumerate(zip(items, members)):
        m.fill(it, 1 if short == k else 0)
    return ops.lib().buctd_conv3x3_wgrad_bf16x6_group(len(members), items, ops.stream_ptr())


@pytest.mark.parametrize("name", list(G.WGRAD_GROUPS))
def test_weight_gradient_group(x6, dev, name):
    ops = x6
    spec = G.WGRAD_GROUPS[name]
    n = len(spec)
    plans, grid, _ = G.wgrad_group_plan(spec)
    runs = []
    for rep in range(2):
        pl = Place(dev, True)
        members = [WgMember(ops, dev, s, n, pl, f"{k} {T.case_id(s[0])}") for k, s in enumerate(spec)]
        ops.check(launch_wgrad(ops, members), f"wgrad group {name}")
        torch.cuda.synchronize()
        pl.check(f"wgrad group {name}")
        runs.append([m.dw.clone() for m in members])
    for k, (m, got, again, wp) in enumerate(zip(members, runs[0], runs[1], plans)):
        what = f"wgrad group {name}, member {m.tag} (accumulate {m.accumulate}, x_bn {m.x_bn}, plan {wp})"
        assert torch.equal(got, again), f"{what}: not run-to-run reproducible"
        # the slabs of the member's plan were written, nothing of the workspace behind them
        used = wp["ws_bytes"] // 4
        assert used == m.ws.numel() and torch.isfinite(m.ws).all(), f"{what}: slabs of its workspace were left unwritten"
        ref, mag, xf = m.reference()
        N, H, W, Ci, Co = m.shape
        w_like = wcl(torch.empty(Co, Ci, 3, 3)).to(dev)
        xfd, dyd = xf.to(dev), nhwc(m.dyc).to(dev)
        dw32 = in_fp32(ops, lambda: ops.conv_wgrad(xfd, dyd, w_like, 1, 1))
        got_l = got.permute(0, 3, 1, 2)                       # logical [Co][Ci][3][3]
        prev_l = m.prev.permute(0, 3, 1, 2).to(dev)
        check_wgrad(what, (m.shape, False), got_l, dw32 + prev_l if m.accumulate else dw32, ref, mag)
        # the member's own launch: another split count, another (fixed) summation order
        x_bn = (m.mean_c.to(dev), m.invstd_c.to(dev), m.bn.weight, m.bn.bias, True) if m.x_bn else None
        out = wcl(m.prev.permute(0, 3, 1, 2)).to(dev) if m.accumulate else None
        one = ops.conv_wgrad(nhwc(m.xc).to(dev), dyd, w_like, 1, 1, out=out, accumulate=m.accumulate, x_bn=x_bn)
        sc = float(one.abs().max())
        d = (got_l - one).abs()
        at = tuple(int(v) for v in torch.unravel_index(d.argmax(), d.shape))
        assert float(d.max()) <= 5e-6 * sc, f"{what}: differs from its single launch by {float(d.max()):.3e} (scale {sc:.3e}) at (co, ci, r, s) = {at}"


@pytest.mark.parametrize("how", ["workspace one byte short", "mixed chunk widths"])
def test_weight_gradient_group_refusals_write_nothing(x6, dev, how):
    from buctd_amd import _C
    ops = x6
    spec = G.WGRAD_GROUPS["cf3-n2"] if how.startswith("workspace") else G.WGRAD_MIXED_CF
    pl = Place(dev, True)
    members = [WgMember(ops, dev, s, len(spec), pl, f"{k}") for k, s in enumerate(spec)]
    before = [(m.dw.clone(), m.ws.clone()) for m in members]
    rc = launch_wgrad(ops, members, short=1 if how.startswith("workspace") else None)
    torch.cuda.synchronize()
    assert rc != 0
    with pytest.raises(_C.BuctdHipError, match="workspace" if how.startswith("workspace") else "chunk width"):
        ops.check(rc, "wgrad group")
    if how.startswith("workspace"):
        assert rc == -3                          # BUCTD_EWORKSPACE
    pl.check(how)
    for m, (dw0, ws0) in zip(members, before):
        same = lambda a, b: torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0))
        assert same(m.dw, dw0) and same(m.ws, ws0), f"{how}: the refused call wrote to member {m.tag}"
