"""Gradient contract of the autograd nodes (buctd_amd/ops.py, ops_seq.py), node by node over the table of
tests/helpers/grad_contract_cases.py: where a parameter gradient is written, in the states the other suites never visit.

a. frozen subsets (every norm affine | every weight | the first weight | all but one parameter; input with and without a
   gradient; with and without a FlatParams arena): a frozen parameter keeps grad None, its arena slot and its value keep
   their bits, the gradient-ready callback never sees it and sees every other parameter once; the trainable parameters
   and the input get the fp64 gradients of the same module with the same requires_grad flags - also when the only
   trainable parameter sits in the last block of a chain whose input needs no gradient;
b. a second backward without zero_grad gives twice the gradient, a mixed state (some gradients set to None, others kept)
   the right sum in both; a mixed state inside one norm layer raises a readable error;
c. with an arena, p.grad aliases the arena view and holds the bits of the run without an arena;
d. a non-contiguous upstream gradient (transposed memory, an expanded scalar) gives the bits of the contiguous one; an
   output of a multi-output node left out of the loss gives the fp64 gradients without that output;
e. three real train steps of a conv-bn-conv-bn-head net with frozen BatchNorm affine parameters under an ungrouped FusedAdam /
   FusedSGD with max_grad_norm, against torch.optim + clip_grad_norm_ in fp64.

Every case first asserts, through a recorder around ops.grad_target, that its backward passes through the functions it
names (`sites`).  Bars: blocks - rel. error against fp64 <= max(5e-6, 4 x the fp32 CPU module's own error), per tensor
(test_gpu_blocks.py); attention and sequence nodes - 2e-5 (test_gpu_attention.py); the 1-D gradients (dgamma, dbeta, biases)
also per element: |d - ref| <= bar x max|ref|.  Bit claims are made only after the baseline equalled itself bit for bit in
two runs: every node of the table is reproducible against itself, none needed the fp64 fall-back."""
import copy
import sys

import pytest
import torch

from tests.helpers import grad_contract_cases as G
from tests.helpers import grad_clip_ref as CR

pytestmark = pytest.mark.gpu
PATTERN = -7.25
NAMES = [c["name"] for c in G.CASES]
_built = {}
_refs = {}


def built(name):
    if name not in _built:
        _built[name] = G.BY_NAME[name]["build"]()
    return _built[name]


def loss_weight(y, ones):
    return torch.ones_like(y) if ones else torch.linspace(-1, 1, y.numel(), dtype=y.dtype).view(y.shape)


def ref_run(name, dt, frozen=(), x_rg=True, drop=None, ones=False):
    """the torch module on the CPU in dtype dt with the given requires_grad flags -> outs, dxs, {name: grad or None};
    computed once per setting and shared"""
    key = (name, dt, tuple(frozen), x_rg, drop, ones)
    if key in _refs:
        return _refs[key]
    b = built(name)
    m = copy.deepcopy(b.ref).to(dt).train()
    for k, p in m.named_parameters():
        p.requires_grad_(k not in frozen)
    xs = [x.to(dt).clone().requires_grad_(x_rg) for x in b.inputs]
    ys = b.ref_fwd(m, xs)
    pairs = [(y, loss_weight(y, ones)) for i, y in enumerate(ys) if i != drop and y.requires_grad]
    if pairs:
        torch.autograd.backward([y for y, _ in pairs], [w for _, w in pairs])
    _refs[key] = ([y.detach() for y in ys], [x.grad for x in xs], {k: p.grad for k, p in m.named_parameters()})
    return _refs[key]


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return (a is None and b is None) or (a is not None and b is not None and a.shape == b.shape and torch.equal(bits(a), bits(b)))


class Session:
    """One copy of the case's module on the device with the given flags, the recorders installed; step() is one forward +
    backward and returns what it left: {"out", "dx", "grad": {name: CPU tensor or None}, "seen": names the gradient-ready
    callback got, "sites": functions that called grad_target}."""

    def __init__(self, dev, name, frozen=(), x_rg=True, arena=False):
        self.dev, self.case, self.b = dev, G.BY_NAME[name], built(name)
        self.frozen, self.x_rg, self.with_arena = set(frozen), x_rg, arena

    def __enter__(self):
        from buctd_amd import engine, ops
        c, b = self.case, self.b
        self.ops = ops
        self.old_math = ops.get_conv_math()
        ops.set_conv_math(c["math"])
        self.old_veto = ops.native_block_veto["fn"]
        if c["veto"]:
            ops.native_block_veto["fn"] = lambda shape: True
        mod = copy.deepcopy(b.mod)
        mod.load_state_dict(b.ref.state_dict(), strict=True)
        self.mod = mod.to(self.dev).train()
        self.params = dict(self.mod.named_parameters())
        assert list(self.params) == [k for k, _ in b.ref.named_parameters()]
        self.old_arena = ops.set_grad_arena(None)
        self.flat = None
        if self.with_arena:
            self.flat = engine.FlatParams(self.mod)          # installs itself as the gradient arena
            self.flat.grad.fill_(PATTERN)
        for k, p in self.params.items():
            p.requires_grad_(k not in self.frozen)
        self.value0 = {k: p.detach().clone() for k, p in self.params.items()}
        self.seen, self.sites = [], set()
        by_id = {id(p): k for k, p in self.params.items()}
        self.old_cb = ops.set_grad_ready_callback(lambda p: self.seen.append(by_id[id(p)]))
        calls, real = G.grad_target_calls(), ops.grad_target

        def recorder(p):
            f = sys._getframe(1)
            self.sites.add(calls[(f.f_code.co_filename.replace("\\", "/").rsplit("/", 1)[-1], f.f_lineno)])
            return real(p)
        self.real_target = real
        ops.grad_target = recorder
        return self

    def __exit__(self, *exc):
        ops = self.ops
        torch.cuda.synchronize()
        ops.grad_target = self.real_target
        ops.set_grad_ready_callback(self.old_cb)
        ops.set_grad_arena(self.old_arena)
        ops.native_block_veto["fn"] = self.old_veto
        ops.set_conv_math(self.old_math)

    def to_dev(self, x):
        return (x.permute(0, 2, 3, 1).contiguous() if self.b.layout == "nchw" else x.clone()).to(self.dev)

    def to_ref(self, t):
        t = t.detach().cpu()
        return t.permute(0, 3, 1, 2) if self.b.layout == "nchw" else t

    def upstream(self, y_ref_shape, form):
        """the loss weight of an output in the device's layout: contiguous, the same values in transposed memory, ones, or
        ones as the expanded scalar that sum().backward() hands down"""
        ones = form in ("ones", "expanded")
        w = self.to_dev(loss_weight(torch.empty(y_ref_shape), ones))
        if form == "permuted":
            w = w.transpose(-1, -2).contiguous().transpose(-1, -2)
            assert not w.is_contiguous()
        if form == "expanded":
            w = torch.ones((), device=self.dev).expand(w.shape)
            assert not w.is_contiguous()
        return w

    def step(self, drop=None, form="contig"):
        b = self.b
        self.seen.clear()
        self.sites.clear()
        xs = [self.to_dev(x).requires_grad_(self.x_rg) for x in b.inputs]
        ys = b.mod_fwd(self.mod, xs)
        pairs = [(y, self.upstream(tuple(self.to_ref(y).shape), form)) for i, y in enumerate(ys) if i != drop and y.requires_grad]
        if pairs:
            torch.autograd.backward([y for y, _ in pairs], [w for _, w in pairs])
        torch.cuda.synchronize()
        return {"node": type(ys[0].grad_fn).__name__ if ys[0].grad_fn is not None else None,
                "out": [self.to_ref(y) for y in ys], "dx": [None if x.grad is None else self.to_ref(x.grad) for x in xs],
                "grad": {k: None if p.grad is None else p.grad.detach().cpu().clone() for k, p in self.params.items()},
                "seen": list(self.seen), "sites": set(self.sites)}


def one_step(dev, name, **kw):
    step_kw = {k: kw.pop(k) for k in ("drop", "form") if k in kw}
    with Session(dev, name, **kw) as s:
        return s.step(**step_kw)


def rel(a, ref):
    return ((a.double() - ref).norm() / ref.norm().clamp_min(1e-30)).item()


def check(name, what, got, ref64, ref32, scale=1.0):
    """the bar of the case's kind, per tensor - and per element for 1-D gradients"""
    kind = G.BY_NAME[name]["kind"]
    ref = ref64 * scale
    e32 = rel(ref32 * scale, ref)
    bar = 2e-5 if kind == "attn" else max(5e-6, 4 * e32)
    err = rel(got, ref)
    print(f"{name}: {what}: {err:.2e} / {bar:.2e} [fp32 CPU {e32:.2e}]")
    assert err <= bar, f"{name}: {what}: rel err vs fp64 {err:.2e} > {bar:.2e} (fp32 CPU {e32:.2e})"
    if what.startswith("d ") and ref.dim() == 1:
        worst = (got.double() - ref).abs().max().item()
        top = ref.abs().max().item()
        assert worst <= bar * top, f"{name}: {what}: element error {worst:.2e} > {bar:.2e} x max|ref| {top:.2e}"


def check_step(name, got, frozen=(), x_rg=True, drop=None, ones=False, scale=None, zero_for_none=False, tag=""):
    """outputs, input gradients and parameter gradients of a step against the fp64 module with the same flags; scale:
    {name: factor} for accumulated gradients; zero_for_none: where the reference has no gradient, an all-zero one passes"""
    y64, dx64, g64 = ref_run(name, torch.float64, frozen, x_rg, drop, ones)
    y32, dx32, g32 = ref_run(name, torch.float32, (), True, drop, ones)
    for i, y in enumerate(got["out"]):
        check(name, f"{tag}out{i}", y, y64[i], y32[i])
    for i, dx in enumerate(got["dx"]):
        if dx64[i] is None:
            assert dx is None or (zero_for_none and not dx.any()), f"{name}: {tag}input {i} got a gradient it should not have"
        else:
            assert dx is not None, f"{name}: {tag}input {i} got no gradient"
            check(name, f"{tag}dx{i}", dx, dx64[i], dx32[i])
    for k, g in got["grad"].items():
        if k in frozen:
            assert g is None, f"{name}: {tag}frozen parameter {k} has .grad set"
        elif g64[k] is None:
            assert g is None or (zero_for_none and not g.any()), f"{name}: {tag}{k} got a gradient, the reference has none"
        else:
            assert g is not None, f"{name}: {tag}{k} got no gradient"
            check(name, f"d {tag}{k}", g, g64[k], g32[k], 1.0 if scale is None else scale[k])
    return g64


def assert_same_step(name, a, b, what, keys=None):
    for i, (p, q) in enumerate(zip(a["out"], b["out"])):
        assert same_bits(p, q), f"{name}: {what}: output {i} differs"
    for i, (p, q) in enumerate(zip(a["dx"], b["dx"])):
        if keys is None or (p is not None and q is not None):
            assert same_bits(p, q), f"{name}: {what}: input gradient {i} differs"
    for k in (a["grad"] if keys is None else keys):
        assert same_bits(a["grad"][k], b["grad"][k]), f"{name}: {what}: gradient of {k} differs"


# ---- a. frozen subsets --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_frozen_parameters_get_no_gradient(dev, name):
    c, b = G.BY_NAME[name], built(name)
    base = one_step(dev, name)
    assert base["node"] == b.node, f"{name}: the output carries {base['node']}, the case is about {b.node}"
    assert set(c["sites"]) <= base["sites"], f"{name}: backward passed {sorted(base['sites'])}, the case names {c['sites']}"
    assert_same_step(name, base, one_step(dev, name), "the baseline is not reproducible against itself")
    g64 = check_step(name, base)
    assert sorted(base["seen"]) == sorted(k for k in g64 if g64[k] is not None), f"{name}: gradient-ready calls {base['seen']}"
    for tag, sub in G.frozen_subsets(b.ref).items():
        for x_rg in (True, False):
            for arena in (False, True):
                what = f"[{tag} frozen, x {'with' if x_rg else 'without'} grad, {'arena' if arena else 'no arena'}] "
                with Session(dev, name, frozen=sub, x_rg=x_rg, arena=arena) as s:
                    got = s.step()
                    g64 = check_step(name, got, sub, x_rg, tag=what)
                    live = [k for k in g64 if k not in sub and g64[k] is not None]
                    # the same kernels on the same operands as with nothing frozen: the same bits
                    assert_same_step(name, got, base, what + "against the run with nothing frozen", keys=live)
                    assert sorted(got["seen"]) == sorted(live), f"{name}: {what}gradient-ready calls {got['seen']}, want {live}"
                    for k in sub:
                        p = s.params[k]
                        assert p.grad is None and same_bits(p.detach(), s.value0[k]), f"{name}: {what}{k}"
                        if arena:
                            slot = s.flat(p)
                            assert same_bits(slot, torch.full_like(slot, PATTERN)), f"{name}: {what}arena slot of {k} was written"
                    if arena:
                        for k in live:
                            assert s.flat.grad_is_arena(s.params[k]), f"{name}: {what}{k}.grad is not the arena view"


# ---- b. accumulation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_second_backward_accumulates(dev, name):
    b = built(name)
    names = [k for k, _ in b.ref.named_parameters()]
    weights = [k for k, p in b.ref.named_parameters() if p.dim() >= 2]
    others = [k for k in names if k not in weights]        # the norm layers' weight AND bias, and the biases
    with Session(dev, name) as s:
        s.step()
        check_step(name, s.step(), scale={k: 2.0 for k in names}, tag="[second backward] ")
    for zeroed in (weights, others):
        if not zeroed:
            continue
        with Session(dev, name) as s:
            s.step()
            for k in zeroed:
                s.params[k].grad = None
            check_step(name, s.step(), scale={k: 1.0 if k in zeroed else 2.0 for k in names},
                       tag=f"[mixed: {len(zeroed)} of {len(names)} zeroed] ")


@pytest.mark.parametrize("name", G.MIXED_NORM)
def test_mixed_state_inside_one_norm_layer_raises(dev, name):
    """one kernel writes dgamma and dbeta with one accumulate flag: weight.grad None next to a kept bias.grad is refused in
    words, not by a bare assert - and neither flag is picked silently"""
    gamma = G.norm_names(built(name).ref)[0]
    assert gamma.endswith("weight")
    with Session(dev, name) as s:
        s.step()
        s.params[gamma].grad = None
        with pytest.raises(RuntimeError, match="one accumulate flag"):
            s.step()


# ---- c. arena -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_arena_holds_the_bits_of_the_run_without_one(dev, name):
    plain = one_step(dev, name)
    with Session(dev, name, arena=True) as s:
        got = s.step()
        assert_same_step(name, got, plain, "arena against no arena")
        for k, p in s.params.items():
            if plain["grad"][k] is None:
                slot = s.flat(p)
                assert p.grad is None and same_bits(slot, torch.full_like(slot, PATTERN)), f"{name}: {k} has no gradient"
                continue
            assert s.flat.grad_is_arena(p), f"{name}: {k}.grad does not alias the arena"
            assert same_bits(s.flat(p).cpu(), plain["grad"][k]), f"{name}: arena slot of {k} differs from the run without an arena"


# ---- d. upstream gradient form ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_non_contiguous_upstream_gradient(dev, name):
    assert_same_step(name, one_step(dev, name, form="permuted"), one_step(dev, name), "transposed-memory dy against contiguous")
    assert_same_step(name, one_step(dev, name, form="expanded"), one_step(dev, name, form="ones"), "expanded scalar dy against ones")


@pytest.mark.parametrize("name", G.MULTI_OUTPUT)
def test_an_output_left_out_of_the_loss(dev, name):
    """dy is None for one output of the node: the other gradients are those of the loss without it (a branch that took no
    part still runs: its parameter gradients are zero where the reference has none)"""
    n_out = len(ref_run(name, torch.float64)[0])
    assert n_out >= 2
    for drop in range(n_out):
        got = one_step(dev, name, drop=drop)
        assert got["node"] == built(name).node
        check_step(name, got, drop=drop, zero_for_none=True, tag=f"[output {drop} left out] ")


# ---- e. downstream: three train steps with frozen BatchNorm affine parameters -----------------------------------------------------
def small_net(project):
    """conv-bn-relu, conv-bn-relu, 1x1 head with bias: torch modules, or the project's with the same state_dict keys"""
    import torch.nn as tnn
    from buctd_amd import nn as bnn
    if not project:
        return tnn.Sequential(tnn.Sequential(tnn.Conv2d(4, 8, 3, 1, 1, bias=False), tnn.BatchNorm2d(8), tnn.ReLU()),
                              tnn.Sequential(tnn.Conv2d(8, 8, 3, 1, 1, bias=False), tnn.BatchNorm2d(8), tnn.ReLU()),
                              tnn.Conv2d(8, 5, 1))
    return bnn.Chain(bnn.ConvBN(bnn.Conv2d(4, 8, 3, 1, 1, bias=False), bnn.BatchNorm2d(8), bnn.ReLU(True)),
                     bnn.ConvBN(bnn.Conv2d(8, 8, 3, 1, 1, bias=False), bnn.BatchNorm2d(8), bnn.ReLU(True)),
                     bnn.Conv2d(8, 5, 1))


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_train_steps_leave_frozen_batchnorm_alone(dev, kind):
    """an ungrouped FusedAdam / FusedSGD with max_grad_norm after real backwards through ConvBnAct and Conv: the frozen gamma
    and beta keep their bits, the total norm and the trainable parameters follow torch.optim + clip_grad_norm_ in fp64 under
    the measured bar of grad_clip_ref / param_groups_ref: max(4 x the fp32 CPU run's error, 2^-23)"""
    from buctd_amd import engine, ops
    torch.manual_seed(31)
    ref = G._shake(small_net(False), 23)
    frozen = set(G.norm_names(ref))
    assert len(frozen) == 4
    max_norm, steps = 0.5, 3
    g = torch.Generator().manual_seed(32)
    xs = [torch.randn(3, 4, 10, 7, generator=g) for _ in range(steps)]
    ws = [torch.randn(3, 5, 10, 7, generator=g) for _ in range(steps)]

    def make_opt(params, dt):
        if kind == "adam":
            return torch.optim.Adam(params, lr=1e-3, foreach=False)
        return torch.optim.SGD(params, lr=0.05, momentum=0.9, weight_decay=1e-4, nesterov=True, foreach=False)
    cpu = {}
    for dt in (torch.float64, torch.float32):
        m = copy.deepcopy(ref).to(dt).train()
        for k, p in m.named_parameters():
            p.requires_grad_(k not in frozen)
        opt = make_opt(list(m.parameters()), dt)
        norms, trail = [], []
        for x, w in zip(xs, ws):
            opt.zero_grad()
            (m(x.to(dt)) * w.to(dt)).sum().backward()
            norms.append(float(torch.nn.utils.clip_grad_norm_(m.parameters(), max_norm)))
            opt.step()
            trail.append({k: p.detach().clone() for k, p in m.named_parameters()})
        cpu[dt] = (norms, trail)
    net = small_net(True)
    net.load_state_dict(ref.state_dict(), strict=True)
    net = net.to(dev).train()
    old_arena = ops.set_grad_arena(None)
    try:
        flat = engine.FlatParams(net)
        params = dict(net.named_parameters())
        for k, p in params.items():
            p.requires_grad_(k not in frozen)
        start = {k: p.detach().cpu().clone() for k, p in params.items()}
        if kind == "adam":
            opt = engine.FusedAdam(flat, lr=1e-3, max_grad_norm=max_norm)
        else:
            opt = engine.FusedSGD(flat, lr=0.05, momentum=0.9, weight_decay=1e-4, nesterov=True, max_grad_norm=max_norm)
        assert not opt.grouped
        for i, (x, w) in enumerate(zip(xs, ws)):
            opt.zero_grad()
            y = net(x.permute(0, 2, 3, 1).contiguous().to(dev))
            assert type(y.grad_fn).__name__ == "ConvBackward"
            (y * w.permute(0, 2, 3, 1).contiguous().to(dev)).sum().backward()
            opt.step()
            torch.cuda.synchronize()
            n64, n32 = cpu[torch.float64][0][i], cpu[torch.float32][0][i]
            got = opt.last_grad_norm.item()
            bar = max(4 * abs(n32 - n64) / n64, CR.FLOOR)
            print(f"{kind} step {i}: total norm {got:.9g} ref {n64:.9g}: {abs(got - n64) / n64:.2e} / {bar:.2e}")
            assert abs(got - n64) / n64 <= bar, f"{kind} step {i}: total norm {got!r}, torch {n64!r} (bar {bar:.2e})"
            for k, p in params.items():
                if k in frozen:
                    assert p.grad is None and same_bits(p.detach().cpu(), start[k]), f"{kind} step {i}: frozen {k} moved"
                    continue
                r64, r32 = cpu[torch.float64][1][i][k], cpu[torch.float32][1][i][k]
                sc = start[k].double().abs() + (r64 - start[k].double()).abs() + 1e-300
                err = ((p.detach().cpu().double() - r64).abs() / sc).max().item()
                bar = max(4 * ((r32.double() - r64).abs() / sc).max().item(), CR.FLOOR)
                print(f"{kind} step {i} {k}: {err:.2e} / {bar:.2e}")
                assert err <= bar, f"{kind} step {i}: {k}: error {err:.2e} > bar {bar:.2e}"
    finally:
        ops.set_grad_arena(old_arena)
