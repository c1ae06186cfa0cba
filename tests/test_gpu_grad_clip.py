"""Gradient-norm clipping on the flat arena (csrc/grad_norm.hip, the _dscale steps of csrc/loss_decode.hip, the max_grad_norm
option of engine.FusedAdam / FusedSGD, engine.clip_grad_norm_, engine.grad_stats, utils.get_network_grad_flow) on the device.
References and bars: tests/helpers/grad_clip_ref.py (fp64 by math.fsum / numpy; torch.optim in float64 on the CPU; none
taken from the kernels).

  reduction     relative error against math.fsum of the fp64 squares <= 2e-10 (n 2^-53 = 1.2e-10 at the longest case); NaN and
                1e30 around and between the runs; two launches and the 16-byte / scalar paths give the same bits
  finalize      1 ulp of fp32 against the fp64 expressions; exactly 1.0f where they give >= 1
  coefficient 1 bit-identical to the optimizers without the option
  clipped step  the measured bar of test_gpu_heatmap_kernels.py for an unclipped step: max(4 x fp32 CPU formula, 2^-23)
  grad_stats    relative 1e-12 against torch in float64

Figures of the MI355X run: DESIGN.md 18.
"""
import copy
import math

import pytest
import torch

from tests.helpers import grad_clip_ref as R

pytestmark = pytest.mark.gpu

MAX_NORM = 0.7


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


# ---- 1. the reduction -------------------------------------------------------------------------------------------------------
def _poisoned(total):
    buf = torch.full((total,), float("nan"))
    buf[1::2] = 1e30
    return buf


def _sumsq(dev, host_buf, runs):
    """-> (the fp64 result as a Python float, its bits); the workspace is exactly as long as asked for, behind it a band"""
    from buctd_amd import ops
    g = host_buf.to(dev)
    need = ops.grad_sumsq_workspace(runs) // 8
    ws = torch.full((need + 8,), -7.0, dtype=torch.float64, device=dev)
    out = torch.full((3,), -7.0, dtype=torch.float64, device=dev)
    ops.grad_sumsq(g, runs, out[1:2], ws[:need])
    torch.cuda.synchronize()
    assert bool((ws[need:] == -7.0).all()) and out[0].item() == -7.0 and out[2].item() == -7.0, "wrote outside its outputs"
    assert torch.equal(bits(g.float()), bits(host_buf.float())), "the gradient buffer was written"
    return out[1].item(), bits(out[1:2])


@pytest.mark.parametrize("n", R.LENGTHS)
def test_sumsq_against_fsum(dev, n):
    gen = torch.Generator().manual_seed(1000 + n % 9973)
    half = max(1, n // 2)
    x = R.log_uniform(2 * n + half, gen)
    worst = 0.0
    layouts = {
        "one": ([(8, 8 + n)], [x[:n]]),
        "odd": ([(9, 9 + n)], [x[:n]]),                       # starts at an odd element: the scalar path
        "three": ([(8, 8 + n), (8 + n + 5, 8 + n + 5 + half), (n + half + 20, 2 * n + half + 20)],
                  [x[:n], x[n:n + half], x[n + half:]]),      # gaps of 5 and 7 elements: aligned and unaligned starts
    }
    ref_one = R.sumsq(x[:n].numpy())
    refs = {"one": ref_one, "odd": ref_one, "three": R.sumsq(x.numpy())}      # the three runs hold all of x
    got_bits = {}
    for kind, (runs, pieces) in layouts.items():
        buf = _poisoned(runs[-1][1] + 9)
        for (s, e), piece in zip(runs, pieces):
            buf[s:e] = piece
        ref = refs[kind]
        got, b = _sumsq(dev, buf, runs)
        again, b2 = _sumsq(dev, buf, runs)
        rel = abs(got - ref) / ref
        worst = max(worst, rel)
        print(f"grad_sumsq n {n} {kind}: {got!r} for {ref!r}, relative error {rel:.3e} (bar 2e-10)")
        assert math.isfinite(got) and rel <= 2e-10, f"n {n} {kind}: relative error {rel:.3e}"
        assert torch.equal(b, b2), f"n {n} {kind}: two launches differ"
        got_bits[kind] = b
    assert torch.equal(got_bits["one"], got_bits["odd"]), f"n {n}: the 16-byte path and the scalar path differ"
    print(f"grad_sumsq n {n}: worst relative error {worst:.3e}")


def test_sumsq_refuses_bad_arguments_before_any_launch(dev):
    from buctd_amd import _C, ops
    g = torch.ones(3 * R.CHUNK, device=dev)
    out = torch.zeros(1, dtype=torch.float64, device=dev)
    ws = torch.zeros(4, dtype=torch.float64, device=dev)
    with pytest.raises(_C.BuctdHipError, match="workspace"):
        ops.grad_sumsq(g, [(0, 3 * R.CHUNK)], out, ws[:2])
    for runs in ([], [(4, 4)], [(0, 3 * R.CHUNK + 1)], [(-1, 5)]):
        with pytest.raises(_C.BuctdHipError):
            ops.grad_sumsq(g, runs, out, ws)
    ops.grad_sumsq(g, [(0, 3 * R.CHUNK)], out, ws[:3])
    assert out.item() == 3.0 * R.CHUNK


# ---- 2. finalize ------------------------------------------------------------------------------------------------------------
def _finalize(dev, sumsq_value, gscale, max_norm):
    from buctd_amd import ops
    s = torch.tensor([sumsq_value], dtype=torch.float64).to(dev)
    coef = torch.full((3,), -7.0, device=dev)
    norm = torch.full((3,), -7.0, device=dev)
    ops.grad_clip_coef(s, gscale, max_norm, coef[1:2], norm[1:2])
    assert coef[0].item() == coef[2].item() == norm[0].item() == norm[2].item() == -7.0
    return coef[1:2].cpu(), norm[1:2].cpu()


@pytest.mark.parametrize("gscale", [1.0, 0.5])
@pytest.mark.parametrize("factor", [0.5, 1.0, 4.0])
def test_finalize_against_the_fp64_expressions(dev, factor, gscale):
    s = (factor * MAX_NORM / gscale) ** 2
    total, c = R.norm_coef(s, MAX_NORM, gscale)
    coef, norm = _finalize(dev, s, gscale, MAX_NORM)
    print(f"finalize {factor} x max_norm, gscale {gscale}: coef {coef.item()!r} for {c!r}, norm {norm.item()!r} for {total!r}")
    assert R.within_one_ulp(coef, c) and R.within_one_ulp(norm, total)
    assert (c < 1.0) == (factor >= 1.0)
    if c >= 1.0:
        assert coef.item() == 1.0


def test_a_non_finite_gradient_gives_a_non_finite_norm(dev):
    """reduction and finalize only: nothing is stepped"""
    from buctd_amd import ops
    for bad, want_coef in ((float("inf"), 0.0), (float("-inf"), 0.0), (float("nan"), float("nan"))):
        g = torch.randn(R.CHUNK + 77)
        g[R.CHUNK + 3] = bad
        runs = [(0, g.numel())]
        out = torch.zeros(1, dtype=torch.float64, device=dev)
        ws = torch.zeros(ops.grad_sumsq_workspace(runs) // 8, dtype=torch.float64, device=dev)
        ops.grad_sumsq(g.to(dev), runs, out, ws)
        coef, norm = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
        ops.grad_clip_coef(out, 1.0, MAX_NORM, coef, norm)
        assert not math.isfinite(norm.item()), bad
        assert coef.item() == want_coef or (math.isnan(want_coef) and math.isnan(coef.item())), (bad, coef.item())


# ---- 3 - 6. the optimizers --------------------------------------------------------------------------------------------------
def _net():
    torch.manual_seed(21)
    net = torch.nn.Sequential(torch.nn.Conv2d(4, 8, 3), torch.nn.BatchNorm2d(8), torch.nn.Linear(10, 6))
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.randn_like(p) * 0.01)       # small, so that an update of about lr is a visible part of p
    return net


def _grads(net, gen, norm=None):
    gs = [torch.randn(p.shape, generator=gen) for p in net.parameters()]
    if norm is not None:
        k = norm / math.sqrt(R.sumsq([g.numpy() for g in gs]))
        gs = [(g.double() * k).float() for g in gs]
    return gs


def _make(kind, flat, **kw):
    from buctd_amd import engine
    if kind == "adam":
        lr, b1, b2, eps = R.ADAM_HYPER
        return engine.FusedAdam(flat, lr=lr, betas=(b1, b2), eps=eps, **kw)
    lr, mu, wd = R.SGD_HYPER
    return engine.FusedSGD(flat, lr=lr, momentum=mu, weight_decay=wd, nesterov=(kind == "nesterov"), **kw)


def _state(opt):
    out = {"p": opt.flat.flat.clone()}
    if hasattr(opt, "exp_avg"):
        out.update(m=opt.exp_avg.clone(), v=opt.exp_avg_sq.clone())
    else:
        out.update(buf=opt.buf.clone())
    return out


def _per_param(opt, name):
    """the optimizer's state of every parameter as one fp32 CPU vector, in parameter order and logical element order"""
    if name == "p":
        return torch.cat([p.detach().cpu().flatten() for p in opt.flat.params])
    key = {"m": "exp_avg", "v": "exp_avg_sq", "buf": "momentum_buffer"}[name]
    sd = opt.state_dict()["state"]
    return torch.cat([sd[i][key].cpu().flatten() for i in range(len(opt.flat.params))])


KINDS = ["adam", "sgd", "nesterov"]


@pytest.mark.parametrize("kind", KINDS)
def test_coefficient_one_returns_the_bits_of_the_plain_step(dev, kind):
    from buctd_amd import engine
    net = _net()
    twins = [copy.deepcopy(net).to(dev) for _ in range(2)]
    plain = _make(kind, engine.FlatParams(twins[0]))
    clipped = _make(kind, engine.FlatParams(twins[1]), max_grad_norm=1e30)
    gen = torch.Generator().manual_seed(3)
    for _ in range(2):
        gs = _grads(net, gen)
        for opt in (plain, clipped):
            opt.zero_grad()
            for q, g in zip(opt.flat.params, gs):
                q.grad = g.to(dev)
            opt.step()
        assert clipped.last_clip_coef.item() == 1.0 and plain.last_clip_coef is None
        want = math.sqrt(R.sumsq([g.numpy() for g in gs]))
        assert R.within_one_ulp(clipped.last_grad_norm.cpu(), want)
        a, b = _state(plain), _state(clipped)
        for k in a:
            assert torch.equal(bits(a[k]), bits(b[k])), f"{kind}: {k} differs from the optimizer without the option"
    assert not torch.equal(_per_param(clipped, "p"), torch.cat([p.detach().flatten() for p in net.parameters()]))


@pytest.mark.parametrize("gscale", [1.0, 0.5])
@pytest.mark.parametrize("kind", KINDS)
def test_clipped_steps_against_torch_in_float64(dev, kind, gscale):
    """three steps, gradient norms 10 x, 0.1 x and 3 x max_norm (of the gradient the step applies: with gscale 0.5, handed
    over by a grad_sync, the arena holds twice that), against clip_grad_norm_ + torch.optim in float64 on the CPU"""
    from buctd_amd import engine
    net = _net()
    twin = copy.deepcopy(net).to(dev)
    sync = {} if gscale == 1.0 else {"grad_sync": lambda: gscale}
    fused = _make(kind, engine.FlatParams(twin), max_grad_norm=MAX_NORM, **sync)
    ref_params = [torch.nn.Parameter(p.detach().double()) for p in net.parameters()]
    if kind == "adam":
        lr, b1, b2, eps = R.ADAM_HYPER
        ref = torch.optim.Adam(ref_params, lr=lr, betas=(b1, b2), eps=eps)
        names = ("p", "m", "v")
    else:
        lr, mu, wd = R.SGD_HYPER
        ref = torch.optim.SGD(ref_params, lr=lr, momentum=mu, weight_decay=wd, nesterov=(kind == "nesterov"))
        names = ("p", "buf")
    cat = lambda ts: torch.cat([t.detach().flatten() for t in ts])      # noqa: E731
    p0 = cat(ref_params).clone()
    s32 = {k: (p0.float() if k == "p" else torch.zeros_like(p0, dtype=torch.float32)) for k in names}
    moved = torch.zeros_like(p0)
    gen = torch.Generator().manual_seed(17)
    for step, factor in enumerate((10.0, 0.1, 3.0), start=1):
        gs = _grads(net, gen, norm=factor * MAX_NORM / gscale)
        total, coef = R.norm_coef(R.sumsq([g.numpy() for g in gs]), MAX_NORM, gscale)
        assert (coef < 1.0) == (factor > 1.0)
        # float64 reference: torch clips the gradient the step applies, then steps
        was = cat(ref_params).clone()
        for q, g in zip(ref_params, gs):
            q.grad = g.double() * gscale
        got_total = torch.nn.utils.clip_grad_norm_(ref_params, MAX_NORM)
        assert abs(got_total.item() - total) <= 1e-13 * total
        ref.step()
        moved += (cat(ref_params) - was).abs()
        # the fp32 formula in the kernel's order, on its own state
        scale = R.f32(R.f32(gscale) * R.f32(coef))
        g32 = torch.cat([g.flatten() for g in gs])
        if kind == "adam":
            s32["p"], s32["m"], s32["v"] = R.adam32(s32["p"], g32, s32["m"], s32["v"], step, scale)
        else:
            s32["p"], s32["buf"] = R.sgd32(s32["p"], g32, s32["buf"], kind == "nesterov", scale)
        # the engine
        fused.zero_grad()
        for q, g in zip(fused.flat.params, gs):
            q.grad = g.to(dev)
        fused.step()
        assert R.within_one_ulp(fused.last_grad_norm.cpu(), total), (fused.last_grad_norm.item(), total)
        assert R.within_one_ulp(fused.last_clip_coef.cpu(), coef), (fused.last_clip_coef.item(), coef)
        key = {"m": "exp_avg", "v": "exp_avg_sq", "buf": "momentum_buffer"}
        for name in names:
            r64 = cat(ref_params) if name == "p" else cat([ref.state[q][key[name]] for q in ref_params])
            if name == "p" and kind == "adam":
                sc = p0.abs() + moved                  # a difference: relative to |p| before and the updates so far
            else:
                sc = r64.abs().max().clamp_min(1e-300)
            err = ((_per_param(fused, name).double() - r64).abs() / sc).max().item()
            e32 = ((s32[name].double() - r64).abs() / sc).max().item()
            bar = max(4 * e32, R.FLOOR)
            print(f"{kind} gscale {gscale} step {step} ({factor} x max_norm) {name}: {err:.3e} / {bar:.3e} [fp32 {e32:.3e}]")
            assert err <= bar, f"{kind} step {step} {name}: error {err:.3e} > bar {bar:.3e} (fp32 CPU formula: {e32:.3e})"


@pytest.mark.parametrize("kind", KINDS)
def test_the_norm_is_taken_behind_the_gradient_scale(dev, kind):
    """grad_sync returns 0.5: the step on g equals, bit for bit, the step without a scale on g / 2 (halving is exact) - with
    the norm of the unscaled gradient the two coefficients would differ by a factor of two"""
    from buctd_amd import engine
    net = _net()
    twins = [copy.deepcopy(net).to(dev) for _ in range(2)]
    scaled = _make(kind, engine.FlatParams(twins[0]), max_grad_norm=MAX_NORM, grad_sync=lambda: 0.5)
    halved = _make(kind, engine.FlatParams(twins[1]), max_grad_norm=MAX_NORM)
    gen = torch.Generator().manual_seed(29)
    for factor in (10.0, 0.1, 3.0):
        gs = _grads(net, gen, norm=factor * MAX_NORM * 2.0)
        for opt, k in ((scaled, 1.0), (halved, 0.5)):
            opt.zero_grad()
            for q, g in zip(opt.flat.params, gs):
                q.grad = (g * k).to(dev)
            opt.step()
        want = 0.5 * math.sqrt(R.sumsq([g.numpy() for g in gs]))
        assert R.within_one_ulp(scaled.last_grad_norm.cpu(), want), (scaled.last_grad_norm.item(), want)
        assert torch.equal(bits(scaled.last_grad_norm), bits(halved.last_grad_norm))
        assert torch.equal(bits(scaled.last_clip_coef), bits(halved.last_clip_coef))
        a, b = _state(scaled), _state(halved)
        for k in a:
            assert torch.equal(bits(a[k]), bits(b[k])), f"{kind} at {factor} x max_norm: {k} differs"


class _Idle(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Conv2d(3, 8, 3)
        self.frozen = torch.nn.Parameter(torch.randn(7, 5), requires_grad=False)
        self.unused = torch.nn.Linear(6, 3)
        self.b = torch.nn.Linear(9, 4)


@pytest.mark.parametrize("kind", KINDS)
def test_a_parameter_without_gradient_neither_enters_the_norm_nor_moves(dev, kind):
    """p.grad is None and the arena slot holds 1e6.  A frozen parameter (requires_grad False) keeps that slot through
    collect(): the runs of the reduction and of FusedSGD leave it out.  FusedAdam steps the whole arena (its docstring), so
    there the case is a trainable parameter that received no gradient: collect() zeroes its slot, the runs leave it out."""
    from buctd_amd import engine
    torch.manual_seed(31)
    net = _Idle()
    twin = copy.deepcopy(net).to(dev)
    flat = engine.FlatParams(twin)
    fused = _make(kind, flat, max_grad_norm=MAX_NORM)
    idle = [twin.unused.weight, twin.unused.bias] + ([twin.frozen] if kind != "adam" else [])
    before = [p.detach().clone() for p in idle]
    gen = torch.Generator().manual_seed(37)
    for _ in range(2):
        fused.zero_grad()
        gs = []
        for n, q in twin.named_parameters():
            if n.startswith(("frozen", "unused")):
                continue
            g = torch.randn(q.shape, generator=gen)
            gs.append(g)
            q.grad = g.to(dev)
        for p in idle:
            flat(p).fill_(1e6)
        fused.step()
        want = math.sqrt(R.sumsq([g.numpy() for g in gs]))
        assert R.within_one_ulp(fused.last_grad_norm.cpu(), want), (fused.last_grad_norm.item(), want)
        for p, b in zip(idle, before):
            assert torch.equal(bits(p), bits(b)), "a parameter without a gradient moved"
    assert not torch.equal(twin.a.weight.detach().cpu(), net.a.weight.detach())


# ---- 7. engine.clip_grad_norm_ ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", [0.5, 3.0])
def test_clip_grad_norm_scales_the_arena_in_place(dev, factor):
    from buctd_amd import engine
    net = _net()
    twin = copy.deepcopy(net).to(dev)
    flat = engine.FlatParams(twin)
    opt = _make("adam", flat)
    gs = _grads(net, torch.Generator().manual_seed(41), norm=factor * MAX_NORM)
    for q, g in zip(flat.params, gs):
        q.grad = g.to(dev)
    total, coef = R.norm_coef(R.sumsq([g.numpy() for g in gs]), MAX_NORM)
    norm = engine.clip_grad_norm_(flat, MAX_NORM)
    assert norm.dim() == 0 and norm.is_cuda and R.within_one_ulp(norm.cpu(), total)
    for q, g in zip(flat.params, gs):
        assert flat.grad_is_arena(q)
        if coef == 1.0:
            assert torch.equal(bits(q.grad), bits(g)), "a gradient below max_norm is left as it is"
        else:
            assert R.within_one_ulp(q.grad.cpu(), g.double() * coef)
    opt.step()                                   # the loop of the reference goes on: step() applies the clipped gradient
    assert opt.last_grad_norm is None
    synced = _make("sgd", engine.FlatParams(copy.deepcopy(net).to(dev)), grad_sync=lambda: 1.0)
    with pytest.raises(RuntimeError, match="max_grad_norm"):
        engine.clip_grad_norm_(synced.flat, MAX_NORM)


# ---- 8. grad_stats / get_network_grad_flow ----------------------------------------------------------------------------------
class _Sizes(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.one = torch.nn.Parameter(torch.randn(1))
        self.conv = torch.nn.Conv2d(5, 7, 3)
        self.p64 = torch.nn.Parameter(torch.randn(64))
        self.frozen = torch.nn.Parameter(torch.randn(33), requires_grad=False)
        self.p65 = torch.nn.Parameter(torch.randn(5, 13))
        self.big = torch.nn.Linear(220, 300)          # 66000 > 2^16 elements


def test_grad_stats_and_grad_flow_against_torch_in_float64(dev):
    from buctd_amd import engine
    from buctd_amd.utils.utils import get_network_grad_flow
    torch.manual_seed(43)
    net = _Sizes()
    twin = copy.deepcopy(net).to(dev)
    flat = engine.FlatParams(twin)
    gen = torch.Generator().manual_seed(47)
    for p, q in zip(net.parameters(), twin.parameters()):
        if p.requires_grad:
            p.grad = R.log_uniform(p.numel(), gen, -6.0, 3.0).view(p.shape)
            q.grad = p.grad.to(dev)
    stats = engine.grad_stats(flat)
    assert sorted(stats) == ["abs_mean", "norm"]
    flow64 = flow32 = 0.0
    for i, (p, q) in enumerate(zip(net.parameters(), flat.params)):
        for key in ("abs_mean", "norm"):
            assert stats[key].dtype == torch.float64 and stats[key].is_cuda and stats[key].shape == (len(flat.params),)
        if not p.requires_grad:
            assert stats["abs_mean"][i].item() == 0.0 and stats["norm"][i].item() == 0.0, "a slot nothing wrote holds zeros"
            continue
        g = p.grad.double()
        for key, want in (("abs_mean", g.abs().mean().item()), ("norm", g.norm().item())):
            got = stats[key][i].item()
            print(f"grad_stats {key} of {tuple(p.shape)}: relative error {abs(got - want) / want:.3e}")
            assert abs(got - want) <= 1e-12 * want, (key, tuple(p.shape), got, want)
        flow64 += g.abs().mean().item()
    for name, param in net.named_parameters():          # the reference's loop (lib/utils/utils.py:293-300)
        if param.requires_grad:
            flow32 += param.grad.abs().mean().item()
    flow = get_network_grad_flow(twin)
    assert isinstance(flow, float) and abs(flow - flow64) <= 1e-12 * flow64 and abs(flow - flow32) <= 1e-6 * flow32
    assert abs(get_network_grad_flow(engine.DataParallel(twin)) - flow64) <= 1e-6 * flow64


# ---- 9. StepGraph -----------------------------------------------------------------------------------------------------------
def test_replayed_clipped_steps_equal_eager_clipped_steps(dev):
    """the optimizer step - reduction, finalize and the _dscale kernel with it - stays outside the captured graph: two replays
    with a clip that bites equal two eager steps bit for bit"""
    from buctd_amd import engine
    from tests.test_gpu_step_graph import _batch, _pair, _prenet_cfg
    cfg = _prenet_cfg()
    ((eager, eopt), (graphed, gopt)), crit = _pair(cfg, dev)
    eopt.max_grad_norm = gopt.max_grad_norm = 1e-5
    step = engine.StepGraph(graphed, crit, gopt, warmup=1)
    for i in range(3):
        x, t, w = _batch(cfg, 4, 300 + i, dev)
        engine.ops.set_grad_arena(eopt.flat)
        loss_e = crit(eager(x), t, w)
        eopt.zero_grad()
        loss_e.backward()
        eopt.step()
        engine.ops.set_grad_arena(gopt.flat)
        _, loss_g = step(x, t, w)
        assert torch.equal(loss_e.detach(), loss_g.detach()), i
        assert 0.0 < eopt.last_clip_coef.item() < 1.0, "the clip bites"
        assert torch.equal(bits(eopt.last_grad_norm), bits(gopt.last_grad_norm)), i
        assert torch.equal(bits(eopt.last_clip_coef), bits(gopt.last_clip_coef)), i
    assert step.replays == 2
    assert torch.equal(eopt.flat.flat, gopt.flat.flat)
    assert torch.equal(eopt.exp_avg, gopt.exp_avg) and torch.equal(eopt.exp_avg_sq, gopt.exp_avg_sq)
