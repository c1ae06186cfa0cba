"""Parameter groups on the flat arena, on the device: the grouped step kernels (csrc/optim_groups.hip) bit for bit against
the plain entry points on the same slices and, with weight decay, against torch.optim in float64; the grouped FusedAdam /
FusedSGD against the plain ones and against torch.optim.Adam / AdamW / SGD with the same groups in float64; the cached chunk
table; get_last_layer_optimizer (reference lib/utils/utils.py:277-290) on a small pose_hrnet.

Bars: bit identity wherever the plain kernels compute the same thing; otherwise the project's measured bar
(test_gpu_heatmap_kernels.py): the same formula in fp32 on the CPU is measured against fp64, bar = max(4 x that, 2^-23), p
relative to |p| before + the updates so far, moments relative to their largest element.  Every case prints
error / bar [fp32 CPU error]."""
import copy
import ctypes as C

import pytest
import torch

from tests.helpers import param_groups_ref as R

pytestmark = pytest.mark.gpu


def bits(t):
    return t.contiguous().view(torch.int32)


def P(t, off=0):
    return None if t is None else t.data_ptr() + 4 * off


def stream():
    from buctd_amd import _C
    return _C.stream_ptr()


def ok(rc, what):
    from buctd_amd import _C
    _C.check(rc, what)


def table_of(spans, owners, total, dev):
    from buctd_amd import ops
    return ops.step_chunk_table(ops.step_chunks(spans, owners, total), dev)


def operands(spans, total, seed, names):
    """{name: fp32 CPU buffer}: NaN and 1e30 outside the spans, values inside (v and nothing else non-negative)"""
    gen = torch.Generator().manual_seed(seed)
    out = {}
    for name in names:
        t = R.poison(total)
        for s, e in spans:
            x = torch.randn(e - s, generator=gen)
            t[s:e] = {"p": x * 0.01, "g": x, "m": x * 0.1, "v": x.abs() * 0.01, "buf": x}[name]
        out[name] = t
    return out


def adam_groups(G, wd=0.0, decoupled=0):
    from buctd_amd import _C
    arr = (_C.AdamGroup * G)()
    for k, t in enumerate(arr):
        t.lr, t.beta1, t.beta2, t.eps, t.step = R.adam_hyper(k)
        t.weight_decay, t.decoupled = wd, decoupled
    return arr


def sgd_groups(G):
    from buctd_amd import _C
    arr = (_C.SgdGroup * G)()
    for k, t in enumerate(arr):
        t.lr, t.momentum, t.nesterov, t.weight_decay = R.sgd_hyper(k)
    return arr


def span_owners(nspans, G):
    """group of every span; with more than one group the last group owns no span"""
    return [k % max(G - 1, 1) for k in range(nspans)]


# ---- 1. kernels: bit identity with the plain entry points ---------------------------------------------------------------------
@pytest.mark.parametrize("with_coef", [False, True], ids=["plain", "dscale"])
@pytest.mark.parametrize("G", [1, 2, 3, 16])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_grouped_step_returns_the_bits_of_the_plain_entry_points(dev, kind, G, with_coef):
    from buctd_amd import _C
    lib = _C.lib()
    lengths = R.SPAN_LENGTHS * (3 if G == 16 else 1)
    spans, total = R.layout(lengths)
    owners = span_owners(len(spans), G)
    names = ("p", "g", "m", "v") if kind == "adam" else ("p", "g", "buf")
    host = operands(spans, total, 100 + G, names)
    table = table_of(spans, owners, total, dev)
    coef = torch.tensor([0.37], device=dev) if with_coef else None
    gscale = 0.5
    groups = adam_groups(G) if kind == "adam" else sgd_groups(G)

    def grouped():
        d = {k: v.to(dev) for k, v in host.items()}
        if kind == "adam":
            ok(lib.buctd_adam_step_groups(P(d["p"]), P(d["g"]), P(d["m"]), P(d["v"]), P(table), table.numel() // 16, groups, G,
                                          gscale, P(coef), stream()), "adam_step_groups")
        else:
            ok(lib.buctd_sgd_step_groups(P(d["p"]), P(d["g"]), P(d["buf"]), P(table), table.numel() // 16, groups, G, gscale,
                                         P(coef), stream()), "sgd_step_groups")
        return d
    got, again = grouped(), grouped()
    want = {k: v.to(dev) for k, v in host.items()}
    for (s, e), k in zip(spans, owners):
        t = groups[k]
        if kind == "adam":
            a = (P(want["p"], s), P(want["g"], s), P(want["m"], s), P(want["v"], s), e - s, t.lr, t.beta1, t.beta2, t.eps, t.step,
                 gscale)
            ok(lib.buctd_adam_step_dscale(*a, P(coef), stream()) if with_coef else lib.buctd_adam_step(*a, stream()), "adam_step")
        else:
            a = (P(want["p"], s), P(want["g"], s), P(want["buf"], s) if t.momentum != 0.0 else None, e - s, t.lr, t.momentum,
                 t.weight_decay, t.nesterov, 0, gscale)
            ok(lib.buctd_sgd_step_dscale(*a, P(coef), stream()) if with_coef else lib.buctd_sgd_step(*a, stream()), "sgd_step")
    torch.cuda.synchronize()
    inside = torch.zeros(total, dtype=torch.bool)
    for s, e in spans:
        inside[s:e] = True
    for name in names:
        g_, w_, a_ = got[name].cpu(), want[name].cpu(), again[name].cpu()
        assert torch.equal(bits(g_)[~inside], bits(host[name])[~inside]), f"{name}: an element outside the spans changed"
        for (s, e), k in zip(spans, owners):
            assert torch.equal(bits(g_[s:e]), bits(w_[s:e])), f"{name}: span [{s}, {e}) of group {k} differs from the plain step"
        assert torch.equal(bits(g_), bits(a_)), f"{name}: two launches from the same state differ"
        assert not bool(torch.isnan(g_[inside]).any())
    assert not torch.equal(got["p"].cpu()[inside], host["p"][inside])
    assert torch.equal(bits(got["g"].cpu()), bits(host["g"])), "the gradient is read-only"


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_more_chunks_than_workgroups(dev, kind):
    """5000 spans of 4 elements, gaps of 4: the grid (at most 4096 workgroups) walks the table a second time.  Reference: the
    plain entry point over the spans packed into one buffer per group (the update is element-wise)."""
    from buctd_amd import _C
    lib = _C.lib()
    n = 5000
    spans = [(8 * k, 8 * k + 4) for k in range(n)]
    owners = [k % 2 for k in range(n)]
    total = 8 * n
    names = ("p", "g", "m", "v") if kind == "adam" else ("p", "g", "buf")
    host = operands(spans, total, 7, names)
    table = table_of(spans, owners, total, dev)
    assert table.numel() // 16 == n
    d = {k: v.to(dev) for k, v in host.items()}
    groups = adam_groups(2) if kind == "adam" else sgd_groups(2)
    if kind == "adam":
        ok(lib.buctd_adam_step_groups(P(d["p"]), P(d["g"]), P(d["m"]), P(d["v"]), P(table), n, groups, 2, 1.0, None, stream()), "")
    else:
        ok(lib.buctd_sgd_step_groups(P(d["p"]), P(d["g"]), P(d["buf"]), P(table), n, groups, 2, 1.0, None, stream()), "")
    idx = torch.arange(total).view(n, 8)[:, :4]
    for k in range(2):
        sel = idx[k::2].reshape(-1)
        pk = {name: host[name][sel].to(dev) for name in names}
        t = groups[k]
        if kind == "adam":
            ok(lib.buctd_adam_step(P(pk["p"]), P(pk["g"]), P(pk["m"]), P(pk["v"]), sel.numel(), t.lr, t.beta1, t.beta2, t.eps,
                                   t.step, 1.0, stream()), "adam_step")
        else:
            ok(lib.buctd_sgd_step(P(pk["p"]), P(pk["g"]), P(pk["buf"]) if t.momentum != 0.0 else None, sel.numel(), t.lr,
                                  t.momentum, t.weight_decay, t.nesterov, 0, 1.0, stream()), "sgd_step")
        for name in names:
            assert torch.equal(bits(d[name].cpu()[sel]), bits(pk[name].cpu())), f"{name}: group {k} differs from the plain step"
    outside = torch.arange(total).view(n, 8)[:, 4:].reshape(-1)
    for name in names:
        assert torch.equal(bits(d[name].cpu()[outside]), bits(host[name][outside])), f"{name}: a gap changed"


# ---- 2. kernels: Adam with weight decay against float64 -----------------------------------------------------------------------
@pytest.mark.parametrize("step", [1, 7])
@pytest.mark.parametrize("decoupled", [0, 1], ids=["coupled", "decoupled"])
def test_adam_weight_decay_against_float64(dev, decoupled, step):
    from buctd_amd import _C
    lib = _C.lib()
    spans, total = R.layout((R.CHUNK + 4, 4, 1028))
    host = operands(spans, total, 40 + step, ("p", "g", "m", "v"))
    if step == 1:
        for s, e in spans:
            host["m"][s:e] = 0.0
            host["v"][s:e] = 0.0
    wd, gscale = 0.1, 0.5
    hyper = R.adam_hyper(1)[:4]
    groups = adam_groups(2, wd, decoupled)
    groups[1].step = step
    d = {k: v.to(dev) for k, v in host.items()}
    table = table_of(spans, [1] * len(spans), total, dev)
    ok(lib.buctd_adam_step_groups(P(d["p"]), P(d["g"]), P(d["m"]), P(d["v"]), P(table), table.numel() // 16, groups, 2, gscale,
                                  None, stream()), "adam_step_groups")
    worst = {}
    for s, e in spans:
        a = [host[k][s:e] for k in "pgmv"]
        r64 = R.torch_adam64(*a, hyper, wd, decoupled, step, gscale)
        r32 = R.adam_formula32(*a, hyper, wd, decoupled, step, gscale)
        scales = (a[0].double().abs() + (r64[0] - a[0].double()).abs(), r64[1].abs().max().clamp_min(1e-300),
                  r64[2].abs().max().clamp_min(1e-300))
        for name, x64, x32, sc in zip("pmv", r64, r32, scales):
            err = ((d[name][s:e].cpu().double() - x64).abs() / sc).max().item()
            e32 = ((x32.double() - x64).abs() / sc).max().item()
            w = worst.setdefault(name, [0.0, 0.0])
            w[0], w[1] = max(w[0], err), max(w[1], e32)
    for name, (err, e32) in sorted(worst.items()):
        print(f"adam_step_groups {'decoupled' if decoupled else 'coupled'} step {step} {name}: {err:.3e} / {R.bar(e32):.3e} "
              f"[fp32 {e32:.3e}]")
    for name, (err, e32) in sorted(worst.items()):
        assert err <= R.bar(e32), f"{name}: error {err:.3e} > bar {R.bar(e32):.3e} (fp32 CPU formula: {e32:.3e})"
    # the decay did something: the same launch without it gives other parameters
    d0 = {k: v.to(dev) for k, v in host.items()}
    g0 = adam_groups(2, 0.0, decoupled)
    g0[1].step = step
    ok(lib.buctd_adam_step_groups(P(d0["p"]), P(d0["g"]), P(d0["m"]), P(d0["v"]), P(table), table.numel() // 16, g0, 2, gscale,
                                  None, stream()), "adam_step_groups")
    s, e = spans[0]
    assert not torch.equal(d0["p"][s:e], d["p"][s:e])


def test_entry_points_refuse_bad_arguments_before_any_launch(dev):
    from buctd_amd import _C
    lib = _C.lib()
    x = torch.zeros(64, device=dev)
    table = table_of([(0, 64)], [0], 64, dev)
    ag, sg = adam_groups(16), sgd_groups(1)       # sgd group 0 has momentum 0.9
    good = [P(x), P(x), P(x), P(x), P(table), 1, ag, 1, 1.0, None, stream()]
    for at in range(5):
        bad = list(good)
        bad[at] = None
        assert lib.buctd_adam_step_groups(*bad) != 0, f"null pointer in argument {at}"
    assert lib.buctd_adam_step_groups(*good[:6], None, 1, 1.0, None, stream()) != 0
    for ng in (0, 17, -1):
        assert lib.buctd_adam_step_groups(*good[:7], ng, 1.0, None, stream()) != 0
        assert lib.buctd_sgd_step_groups(P(x), P(x), P(x), P(table), 1, sg, ng, 1.0, None, stream()) != 0
    for nc in (0, -3):
        assert lib.buctd_adam_step_groups(*good[:5], nc, ag, 1, 1.0, None, stream()) != 0
        assert lib.buctd_sgd_step_groups(P(x), P(x), P(x), P(table), nc, sg, 1, 1.0, None, stream()) != 0
    for at in (0, 1, 3):
        bad = [P(x), P(x), P(x), P(table), 1, sg, 1, 1.0, None, stream()]
        bad[at] = None
        assert lib.buctd_sgd_step_groups(*bad) != 0
    assert lib.buctd_sgd_step_groups(P(x), P(x), None, P(table), 1, sg, 1, 1.0, None, stream()) != 0, "momentum without a buffer"
    assert b"momentum" in lib.buctd_last_error()
    torch.cuda.synchronize()
    assert not bool(x.any())


# ---- 3. engine ---------------------------------------------------------------------------------------------------------------
def conv_bn_conv():
    torch.manual_seed(21)
    net = torch.nn.Sequential()
    net.add_module("stem", torch.nn.Sequential(torch.nn.Conv2d(4, 8, 3), torch.nn.BatchNorm2d(8)))
    net.add_module("mid", torch.nn.Sequential(torch.nn.Conv2d(8, 8, 3), torch.nn.BatchNorm2d(8)))
    net.add_module("side", torch.nn.Linear(10, 6))
    net.add_module("final_layer", torch.nn.Conv2d(8, 5, 1))
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.randn_like(p) * 0.01)
    return net


def grads_of(net, gen):
    return [torch.randn(p.shape, generator=gen) for p in net.parameters()]


def arenas(opt):
    out = {"p": opt.flat.flat}
    if hasattr(opt, "exp_avg"):
        out.update(m=opt.exp_avg, v=opt.exp_avg_sq)
    elif opt.buf is not None:
        out.update(buf=opt.buf)
    return {k: v.clone() for k, v in out.items()}


@pytest.mark.parametrize("clip", [None, 0.5], ids=["noclip", "clip"])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_one_group_over_everything_is_the_plain_optimizer(dev, kind, clip):
    from buctd_amd import engine
    net = conv_bn_conv()
    twins = [copy.deepcopy(net).to(dev) for _ in range(2)]
    flats = [engine.FlatParams(t) for t in twins]
    if kind == "adam":
        plain = engine.FusedAdam(flats[0], lr=1e-3, max_grad_norm=clip)
        grouped = engine.FusedAdam(flats[1], lr=1e-3, max_grad_norm=clip, groups=[{"params": flats[1].params}])
    else:
        kw = dict(lr=0.05, momentum=0.9, weight_decay=1e-4, nesterov=True, max_grad_norm=clip)
        plain = engine.FusedSGD(flats[0], **kw)
        grouped = engine.FusedSGD(flats[1], groups=[{"params": flats[1].params}], **kw)
    gen = torch.Generator().manual_seed(5)
    for _ in range(5):
        gs = grads_of(net, gen)
        for opt in (plain, grouped):
            opt.zero_grad()
            for q, g in zip(opt.flat.params, gs):
                q.grad = g.to(dev)
            opt.step()
        a, b = arenas(plain), arenas(grouped)
        for k in a:
            assert torch.equal(bits(a[k]), bits(b[k])), f"{kind}: {k} differs from the plain optimizer"
        if clip:
            assert torch.equal(plain.last_grad_norm, grouped.last_grad_norm) and grouped.last_clip_coef.item() < 1.0
    assert grouped.table_builds == 1
    assert not torch.equal(grouped.flat.flat.cpu(), torch.zeros(1)) and grouped.grouped and not plain.grouped


def group_options(kind):
    if kind == "sgd":
        return ({"lr": 0.05, "momentum": 0.9, "weight_decay": 0.0, "nesterov": True, "dampening": 0},
                {"lr": 0.01, "momentum": 0.5, "weight_decay": 1e-2, "nesterov": False, "dampening": 0},
                {"lr": 0.02, "momentum": 0.9, "weight_decay": 1e-3, "nesterov": False, "dampening": 0})
    return ({"lr": 1e-2, "betas": (0.8, 0.99), "eps": 1e-8, "weight_decay": 0.0},
            {"lr": 1e-3, "betas": (0.9, 0.999), "eps": 1e-6, "weight_decay": 0.1},
            {"lr": 5e-4, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0.05})


def compare_with_torch(kind, fused, ref, twins64, sim, start, index_groups, tag):
    """stepped parameters and their state against torch in float64 under the measured bar"""
    key_a = "momentum_buffer" if kind == "sgd" else "exp_avg"
    for g in index_groups:
        for i in g["params"]:
            q, r = fused.flat.params[i], twins64[i]
            moved = (r.data - start[i].double()).abs()
            sc = start[i].double().abs() + moved + 1e-300
            err = ((q.detach().cpu().double() - r.data).abs() / sc).max().item()
            e32 = ((sim.p[i].double() - r.data).abs() / sc).max().item()
            print(f"{tag} {kind} parameter {i} p: {err:.3e} / {R.bar(e32):.3e} [fp32 {e32:.3e}]")
            assert err <= R.bar(e32), f"{tag} parameter {i}: error {err:.3e} > bar {R.bar(e32):.3e}"
            st = ref.state.get(r, {})
            for key, arena, s32 in ((key_a, getattr(fused, "exp_avg", None) if kind != "sgd" else fused.buf, sim.a),
                                    ("exp_avg_sq", getattr(fused, "exp_avg_sq", None), sim.b)):
                if st.get(key) is None or arena is None:
                    continue
                x = fused.flat._view(arena, q).cpu().double()
                sc = st[key].abs().max().clamp_min(1e-300)
                err = ((x - st[key]).abs() / sc).max().item()
                e32 = ((s32[i].double() - st[key]).abs() / sc).max().item()
                print(f"{tag} {kind} parameter {i} {key}: {err:.3e} / {R.bar(e32):.3e} [fp32 {e32:.3e}]")
                assert err <= R.bar(e32), f"{tag} parameter {i} {key}: error {err:.3e} > bar {R.bar(e32):.3e}"


@pytest.mark.parametrize("kind", ["adam", "adamw", "sgd"])
def test_three_groups_against_torch_in_float64(dev, kind):
    """head / trunk with decay / a frozen group, and parameters in no group (side.*); five steps.  Frozen and ungrouped
    parameters and their moment slots hold NaN gradients and must stay bit-unchanged."""
    from buctd_amd import engine
    net = conv_bn_conv()
    twin = copy.deepcopy(net).to(dev)
    names = [n for n, _ in net.named_parameters()]
    pick = lambda sub: [i for i, n in enumerate(names) if sub in n]      # noqa: E731
    opts = group_options(kind)
    index_groups = [dict(opts[0], params=pick("final_layer")), dict(opts[1], params=pick("stem")), dict(opts[2], params=pick("mid"))]
    frozen, ungrouped = pick("mid"), pick("side")
    flat = engine.FlatParams(twin)
    for i in frozen:
        flat.params[i].requires_grad = False
    fgroups = [dict({k: v for k, v in g.items() if k != "params"}, params=[flat.params[i] for i in g["params"]])
               for g in index_groups]
    if kind == "sgd":
        fused = engine.FusedSGD(flat, groups=fgroups)
    else:
        fused = engine.FusedAdam(flat, groups=fgroups, decoupled_weight_decay=kind == "adamw")
    for name in ("exp_avg", "exp_avg_sq", "buf"):           # recognisable state in every slot that no step may touch
        arena = getattr(fused, name, None)
        if arena is not None:
            for i in frozen + ungrouped:
                flat._view(arena, flat.params[i]).fill_(0.25)
    before = arenas(fused)
    start = [p.detach().clone() for p in net.parameters()]
    twins64 = [torch.nn.Parameter(p.detach().double().clone()) for p in net.parameters()]
    ref = R.make_torch(kind, twins64, index_groups[:2])       # the frozen group never has a gradient: torch never sees it
    sim = R.Formula32(kind, start, index_groups)
    gen = torch.Generator().manual_seed(9)
    live = index_groups[0]["params"] + index_groups[1]["params"]
    for _ in range(5):
        gs = grads_of(net, gen)
        fused.zero_grad()
        for i in live:
            flat.params[i].grad = gs[i].to(dev)
            twins64[i].grad = gs[i].double()
        for i in frozen + ungrouped:
            flat(flat.params[i]).fill_(float("nan"))        # their slots of the gradient arena
        fused.step()
        ref.step()
        sim.step([gs[i] if i in live else None for i in range(len(gs))])
    compare_with_torch(kind, fused, ref, twins64, sim, start, index_groups[:2], "three groups")
    after = arenas(fused)
    for i in frozen + ungrouped:
        s, e = flat.span(flat.params[i])
        for k in before:
            assert torch.equal(bits(before[k][s:e]), bits(after[k][s:e])), f"{names[i]}: {k} changed"
    assert fused.table_builds == 1
    if kind != "sgd":
        assert fused.group_steps == [5, 5, 0]
    sd = fused.state_dict()
    assert sorted(sd["state"]) == list(range(len(live))), "state exists for the stepped parameters only"


def test_gradual_unfreezing_starts_the_groups_own_counter(dev):
    """the trunk group starts to require gradients at step 3: its bias corrections start there, as torch's per-parameter
    steps do, and the chunk table is rebuilt exactly then"""
    from buctd_amd import engine
    kind = "adam"
    net = conv_bn_conv()
    twin = copy.deepcopy(net).to(dev)
    names = [n for n, _ in net.named_parameters()]
    pick = lambda sub: [i for i, n in enumerate(names) if sub in n]      # noqa: E731
    opts = group_options(kind)
    index_groups = [dict(opts[0], params=pick("final_layer")), dict(opts[1], params=pick("stem") + pick("mid"))]
    flat = engine.FlatParams(twin)
    fused = engine.FusedAdam(flat, groups=[dict({k: v for k, v in g.items() if k != "params"},
                                                params=[flat.params[i] for i in g["params"]]) for g in index_groups])
    start = [p.detach().clone() for p in net.parameters()]
    twins64 = [torch.nn.Parameter(p.detach().double().clone()) for p in net.parameters()]
    ref = R.make_torch(kind, twins64, index_groups)
    sim = R.Formula32(kind, start, index_groups)
    gen = torch.Generator().manual_seed(11)
    ptrs, builds = [], []
    for k in range(1, 6):
        live = index_groups[0]["params"] + (index_groups[1]["params"] if k >= 3 else [])
        gs = grads_of(net, gen)
        fused.zero_grad()
        ref.zero_grad()
        for i in live:
            flat.params[i].grad = gs[i].to(dev)
            twins64[i].grad = gs[i].double()
        fused.step()
        ref.step()
        sim.step([gs[i] if i in live else None for i in range(len(gs))])
        ptrs.append(fused._live.table.data_ptr())
        builds.append(fused.table_builds)
    assert fused.group_steps == [5, 3]
    assert builds == [1, 1, 2, 2, 2], "the table is rebuilt exactly when the live set changes"
    assert ptrs[0] == ptrs[1] and ptrs[2] == ptrs[3] == ptrs[4], "a steady-state step reuses the cached table"
    compare_with_torch(kind, fused, ref, twins64, sim, start, index_groups, "unfreezing")
    for i in pick("side"):
        assert torch.equal(flat.params[i].detach().cpu(), start[i])


def test_a_steady_state_step_is_one_launch_and_no_copy(dev, monkeypatch):
    from buctd_amd import engine, ops
    net = conv_bn_conv().to(dev)
    flat = engine.FlatParams(net)
    fused = engine.FusedAdam(flat, groups=[{"params": flat.params[:4], "lr": 1e-2}, {"params": flat.params[6:]}])
    calls = {"step": 0, "upload": 0, "chunks": 0}
    for name, key in (("adam_step_groups", "step"), ("step_chunk_table", "upload"), ("step_chunks", "chunks")):
        def counted(*a, _f=getattr(ops, name), _k=key, **kw):
            calls[_k] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(ops, name, counted)
    monkeypatch.setattr(ops, "adam_step", lambda *a, **k: pytest.fail("the plain kernel ran in the grouped form"))
    gen = torch.Generator().manual_seed(2)
    for k in range(4):
        fused.zero_grad()
        for q, g in zip(flat.params, grads_of(net, gen)):
            q.grad = g.to(dev)
        fused.step()
        assert calls == {"step": k + 1, "upload": 1, "chunks": 1}
    flat.params[0].grad = None                     # the live set changes: one more table
    fused.step()
    assert calls == {"step": 5, "upload": 2, "chunks": 2} and fused.group_steps == [5, 5]


def test_get_last_layer_optimizer_trains_the_head_alone(dev):
    """the reference's fine-tuning sequence on a small pose_hrnet: every parameter but final_layer.* keeps its bits over three
    train steps, BatchNorm running statistics move, the first step gives final_layer.* the bits of a plain FusedAdam step
    from the same start, and the loss decreases"""
    from oracle import recipes
    from buctd_amd import engine, models
    from buctd_amd.core.loss import JointsMSELoss
    from buctd_amd.utils import utils
    cfg, omodel, x, joints = recipes.build("prenet_w16_96x64")
    tgt, wt = recipes.make_targets(cfg, joints, 77)
    x, tgt, wt = x.to(dev), tgt.to(dev), wt.to(dev)
    nets = []
    for _ in range(2):
        net = models.pose_hrnet.get_pose_net(cfg, is_train=False)
        net.load_state_dict(omodel.state_dict(), strict=True)
        nets.append(net.to(dev).train())
    crit = JointsMSELoss(True)

    def train_step(net, opt):
        from buctd_amd import ops
        ops.set_grad_arena(opt.flat)
        loss = crit(net(x), tgt, wt)
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss.item()
    plain = engine.FusedAdam(engine.FlatParams(nets[1]), lr=cfg.TRAIN.LR)
    train_step(nets[1], plain)
    net = nets[0]
    opt = utils.get_last_layer_optimizer(cfg, net)
    names = [n for n, _ in net.named_parameters()]
    assert sorted(n for n, p in net.named_parameters() if p.requires_grad) == sorted(n for n in names if "final_layer" in n)
    start = {n: p.detach().clone() for n, p in net.named_parameters()}
    stats = {n: b.detach().clone() for n, b in net.named_buffers() if "running" in n}
    losses = [train_step(net, opt)]
    for (n, p), (_, q) in zip(net.named_parameters(), nets[1].named_parameters()):
        if "final_layer" in n:
            assert torch.equal(bits(p.detach()), bits(q.detach())), f"{n}: not the bits of the plain FusedAdam step"
            assert not torch.equal(p.detach(), start[n])
    losses += [train_step(net, opt) for _ in range(2)]
    for n, p in net.named_parameters():
        if "final_layer" not in n:
            assert torch.equal(bits(p.detach()), bits(start[n])), f"{n}: a frozen parameter changed"
    assert any(not torch.equal(b, stats[n]) for n, b in net.named_buffers() if n in stats), "BatchNorm statistics stand still"
    assert losses[2] < losses[1] < losses[0], losses
    assert opt.table_builds == 1 and opt.group_steps == [3]
