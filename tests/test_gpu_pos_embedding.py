"""MODEL.POS_EMBEDDING = 'learnable' trains on the device: buctd_batch_sum (csrc/elementwise.hip) against fp64 through the C
interface, the encoder's parameter gradients against the CPU oracle, the once-per-backward gradient protocol of a parameter
that every encoder layer uses (ops_seq.AddPos), and the TransPose network through the engine (flat arenas, FusedAdam /
FusedSGD, StepGraph, ForwardGraph).

Bars, none taken from the kernels:
  batch_sum   |got - fp64| <= (batch + 1) 2^-24 (|out0| + sum_b |x_b|) per element: first-order bound of a sequential fp32 sum
              of batch (+ 1 when accumulating) terms; small-integer inputs, the 16-byte path against the scalar one and two
              runs of one call: the same bits
  gradients   the project's bar for encoder tensors (tests/test_gpu_models.py): relative error against the fp64 oracle
              <= 5 x (error of the fp32 CPU oracle) + 2e-5, per parameter
  StepGraph   bit-equal to the eager engine (the comparison of tests/test_gpu_step_graph_dropout.py, plus the gradient arena)
"""
import copy
import functools

import pytest
import torch

from tests.helpers.guard_bands import SENTINEL, untouched

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BAND = 256


# ---- the kernel through the C interface ------------------------------------------------------------------------------------
def P(t):
    return t.data_ptr()


def stream():
    from buctd_amd import _C
    return _C.stream_ptr()


def ok(rc, what):
    from buctd_amd import _C
    _C.check(rc, what)


def placed(t, dev, fill, shift):
    """a copy of t on the device between bands of `fill`, `shift` floats off a 16-byte boundary -> (view, allocation, pad)"""
    pad = BAND + shift
    big = torch.full((2 * BAND + 4 + t.numel(),), fill, dtype=torch.float32, device=dev)
    view = big[pad:pad + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 * shift
    return view, big, pad


def run_batch_sum(dev, x, out0, accumulate, shift=0):
    """x [batch, n] read-only between NaN bands, out between sentinel bands -> the result on the host; out starts as out0
    (NaN where the call has to overwrite it)"""
    from buctd_amd import _C
    batch, n = x.shape
    xv, xbig, xpad = placed(x, dev, float("nan"), shift)
    init = out0 if accumulate else torch.full((n,), float("nan"))
    ov, obig, opad = placed(init, dev, SENTINEL, shift)
    ok(_C.lib().buctd_batch_sum(P(xv), batch, n, P(ov), accumulate, stream()), "batch_sum")
    torch.cuda.synchronize()
    assert untouched(obig, opad, n), f"batch_sum {(batch, n)}: the launch wrote outside out"
    assert torch.equal(xv.cpu(), x), f"batch_sum {(batch, n)}: the launch wrote into its input"
    return ov.cpu()


# (batch, n): one thread, one wave with a tail, 16-byte lanes, odd sizes, a full unrolled group of rows and rows beyond it,
# more than one workgroup on either path (scalar with n % 4 = 3), and the grid-stride second trip of either path (the grid
# is capped at 4096 workgroups of 256 threads)
CASES = [(1, 1), (1, 1027), (2, 4), (3, 7), (5, 1024), (33, 1000), (7, 111), (8, 12), (16, 8), (3, 2 * 256 * 4 * 2),
         (4, 2 * 256 * 4 * 2 + 3), (2, 4096 * 256 + 5), (2, 4 * 4096 * 256 + 8)]
ALIGNED = [c for c in CASES if c[1] % 4 == 0]


@functools.lru_cache(maxsize=None)
def operands(batch, n, integers=False):
    g = torch.Generator().manual_seed(1000 * batch + n % 997 + (7 if integers else 0))
    if integers:
        x = torch.randint(-64, 65, (batch, n), generator=g).float()
        out0 = torch.randint(-64, 65, (n,), generator=g).float()
    else:
        x = torch.randn(batch, n, generator=g)
        out0 = torch.randn(n, generator=g)
    return x, out0


@functools.lru_cache(maxsize=None)
def reference(batch, n, accumulate, integers=False):
    """(fp64 sum, sum of magnitudes) per element"""
    x, out0 = operands(batch, n, integers)
    ref, mag = x.double().sum(0), x.double().abs().sum(0)
    if accumulate:
        ref, mag = ref + out0.double(), mag + out0.double().abs()
    return ref, mag


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=str)
def test_batch_sum_against_fp64(dev, case, accumulate):
    batch, n = case
    x, out0 = operands(batch, n)
    ref, mag = reference(batch, n, accumulate)
    got = run_batch_sum(dev, x, out0, accumulate)
    err = (got.double() - ref).abs()
    bar = (batch + 1) * U * mag
    worst = (err / mag.clamp_min(1e-300)).max().item()
    print(f"batch_sum {case} accumulate {accumulate}: worst |err| / sum|terms| {worst:.3e}, bar {(batch + 1) * U:.3e}")
    assert bool((err <= bar).all()), f"batch_sum {case}: |err| / sum|terms| {worst:.3e} > ({batch} + 1) 2^-24"
    again = run_batch_sum(dev, x, out0, accumulate)
    assert torch.equal(got, again), f"batch_sum {case}: two runs differ"


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=str)
def test_batch_sum_of_small_integers_is_exact(dev, case, accumulate):
    batch, n = case
    x, out0 = operands(batch, n, True)
    ref, _ = reference(batch, n, accumulate, True)
    got = run_batch_sum(dev, x, out0, accumulate)
    assert torch.equal(got, ref.float()), f"batch_sum {case}: {(got != ref.float()).sum().item()} of {n} elements differ"


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("case", ALIGNED, ids=str)
def test_batch_sum_scalar_path_returns_the_bits_of_the_16_byte_path(dev, case, accumulate):
    """x and out one float off a 16-byte boundary force the scalar kernel at a size the 16-byte kernel takes"""
    batch, n = case
    x, out0 = operands(batch, n)
    ref, mag = reference(batch, n, accumulate)
    vec = run_batch_sum(dev, x, out0, accumulate)
    scalar = run_batch_sum(dev, x, out0, accumulate, shift=1)
    assert bool(((scalar.double() - ref).abs() <= (batch + 1) * U * mag).all()), f"batch_sum {case}: scalar path beyond the bar"
    assert torch.equal(vec, scalar), f"batch_sum {case}: {(vec != scalar).sum().item()} of {n} elements differ"


def test_batch_sum_refuses_bad_arguments_before_any_launch(dev):
    from buctd_amd import _C
    lib = _C.lib()
    x = torch.ones(2, 8, device=dev)
    out = torch.full((8,), 5.0, device=dev)
    for args in ((None, 2, 8, P(out)), (P(x), 2, 8, None), (P(x), 0, 8, P(out)), (P(x), -1, 8, P(out)), (P(x), 2, 0, P(out)),
                 (P(x), 2, -4, P(out))):
        rc = lib.buctd_batch_sum(*args, 0, stream())
        assert rc != 0, args
        with pytest.raises(_C.BuctdHipError, match="batch_sum"):
            _C.check(rc, "batch_sum")
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())


# ---- the encoder's gradients against the oracle ---------------------------------------------------------------------------
D, HEADS, FF, T, B = 32, 2, 64, 24, 3


def _encoders(layers, dev, seed):
    """(oracle encoder with dropout 0 and randomised vectors, the engine's encoder with its weights on the device, pos [T,1,D],
    tokens [T,B,D], loss weights [T,B,D])"""
    from oracle import models as omodels, recipes
    from buctd_amd.models import transpose_h as th
    torch.manual_seed(seed)
    om = omodels.TransformerEncoder(D, HEADS, FF, layers)
    recipes.set_dropout(om, 0.0)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for k, p in om.named_parameters():
            if p.dim() == 1:            # biases and LayerNorm vectors: away from their 0 / 1 initial values
                p.copy_(torch.randn(p.shape, generator=g) * 0.1 + (1.0 if "norm" in k and k.endswith("weight") else 0.0))
    layer = th.TransformerEncoderLayer(d_model=D, nhead=HEADS, dim_feedforward=FF, dropout=0.0)
    net = th.TransformerEncoder(layer, layers)
    res = net.load_state_dict(om.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    pos = torch.randn(T, 1, D, generator=g)
    src = torch.randn(T, B, D, generator=g)
    wgt = torch.randn(T, B, D, generator=g)
    return om.train(), net.to(dev).train(), pos, src, wgt


def _oracle_grads(om, pos, src, wgt, dtype):
    m = copy.deepcopy(om).to(dtype)
    p = torch.nn.Parameter(pos.to(dtype))
    (m(src.to(dtype), pos=p) * wgt.to(dtype)).sum().backward()
    grads = {k: q.grad.detach() for k, q in m.named_parameters()}
    grads["pos"] = p.grad.detach()
    return grads


def _engine_backward(net, pos, src, wgt, dev):
    """tokens are batch-major on the engine: [B, T, D]"""
    out = net(src.transpose(0, 1).contiguous().to(dev), pos=pos)
    (out * wgt.transpose(0, 1).contiguous().to(dev)).sum().backward()


def relerr(a, ref):
    return (a.detach().cpu().double() - ref).norm().item() / ref.norm().item()


@pytest.fixture
def plain_sink():
    """gradients go to fresh tensors and nobody is told: no arena, no readiness callback; both are put back afterwards"""
    from buctd_amd import ops
    arena, cb = ops.set_grad_arena(None), ops.set_grad_ready_callback(None)
    yield ops
    ops.set_grad_arena(arena)
    ops.set_grad_ready_callback(cb)


def test_encoder_gradients_match_the_oracle(dev, plain_sink):
    om, net, pos0, src, wgt = _encoders(2, dev, 41)
    g64, g32 = _oracle_grads(om, pos0, src, wgt, torch.float64), _oracle_grads(om, pos0, src, wgt, torch.float32)
    pos = torch.nn.Parameter(pos0.to(dev))
    _engine_backward(net, pos, src, wgt, dev)
    got = dict(net.named_parameters())
    got["pos"] = pos
    assert sorted(got) == sorted(g64)
    for k in sorted(g64):
        g = got[k].grad
        assert g is not None, f"{k}: no gradient"
        assert g.shape == got[k].shape
        eh, ec = relerr(g, g64[k]), relerr(g32[k], g64[k])
        print(f"{k}: hip {eh:.2e} / fp32 CPU {ec:.2e}")
        assert eh <= 5 * ec + 2e-5, f"encoder gradient {k}: hip {eh:.2e} vs fp32 CPU {ec:.2e}"
    # a gradient that is already there is added to, in place
    known = torch.randn(T, 1, D, generator=torch.Generator().manual_seed(43))
    for p in net.parameters():
        p.grad = None
    held = pos.grad = known.to(dev)
    _engine_backward(net, pos, src, wgt, dev)
    assert pos.grad is held and pos.grad.data_ptr() == held.data_ptr()
    want = known.double() + g64["pos"]
    eh, ec = relerr(pos.grad, want), relerr(known + g32["pos"], want)
    print(f"known + pos gradient: hip {eh:.2e} / fp32 CPU {ec:.2e}")
    assert eh <= 5 * ec + 2e-5, f"known + gradient: hip {eh:.2e} vs fp32 CPU {ec:.2e}"


# ---- once per backward ----------------------------------------------------------------------------------------------------
def test_gradient_is_reported_once_per_backward_after_its_last_piece(dev, plain_sink):
    """a readiness callback as engine.DataParallel installs it: per backward pass of a 3-layer encoder it fires once for the
    embedding, and the gradient it sees there is the finished one; forwards that are never backpropagated (eval mode with
    the graph kept alive, no_grad) in between change nothing"""
    _, net, pos0, src, wgt = _encoders(3, dev, 51)
    pos = torch.nn.Parameter(pos0.to(dev))
    x = src.transpose(0, 1).contiguous().to(dev)
    seen = []

    def ready(p):
        if p is pos:
            seen.append(p.grad.detach().clone())

    plain_sink.set_grad_ready_callback(ready)
    finals, stray = [], []
    for i in range(2):
        for p in list(net.parameters()) + [pos]:
            p.grad = None
        # the model hands the encoder a [T, D] view of the [T, 1, D] parameter
        _engine_backward(net, pos.view(T, D), src, wgt, dev)
        finals.append(pos.grad.detach().clone())
        assert len(seen) == i + 1, f"pass {i}: the embedding was reported {len(seen) - i} times"
        assert pos.grad.shape == (T, 1, D)
        net.eval()
        stray.append(net(x, pos=pos.view(T, D)))            # graph recorded, kept, never backpropagated
        net.train()
        with torch.no_grad():
            net(x, pos=pos.view(T, D))
    assert len(seen) == 2
    for got, want in zip(seen, finals):
        assert torch.equal(got, want), "the embedding was reported before its last piece"
    assert float(finals[0].abs().max()) > 0 and float(finals[1].abs().max()) > 0


def test_attention_maps_between_the_passes_do_not_disturb_the_report(dev):
    """the whole network, its gradients in the engine's arena: TransPoseH.attention_maps between a forward and its backward
    and between two passes; the embedding is reported once per pass, finished"""
    from buctd_amd import engine, ops
    from buctd_amd.core.loss import JointsMSELoss
    cfg = _cfg("learnable")
    net = _net(cfg, dev)
    opt = engine.get_optimizer(cfg, engine.DataParallel(net))
    net.train()
    pe = net.pos_embedding
    crit = JointsMSELoss(True)
    x, t, w = _batch(cfg, 2, 310, dev)
    seen = []
    old = ops.set_grad_ready_callback(lambda p: seen.append(p.grad.detach().clone()) if p is pe else None)
    try:
        for i in range(2):
            loss = crit(net(x), t, w)
            net.attention_maps(x, query="pred")
            opt.zero_grad()
            loss.backward()
            assert len(seen) == i + 1, f"pass {i}: the embedding was reported {len(seen) - i} times"
            assert opt.flat.grad_is_arena(pe) and torch.equal(seen[i], pe.grad)
            assert float(pe.grad.abs().max()) > 0
            net.attention_maps(x, query=None)
            assert net.training
    finally:
        ops.set_grad_ready_callback(old)


def test_second_backward_through_a_retained_graph_adds_and_reports_again(dev, plain_sink):
    from buctd_amd import ops_seq
    pos = torch.nn.Parameter(torch.randn(T, 1, D, device=dev))
    x = torch.randn(B, T, D, device=dev, requires_grad=True)
    dy = torch.randn(B, T, D, device=dev)
    seen = []
    plain_sink.set_grad_ready_callback(lambda p: seen.append(p.grad.detach().clone()))
    ops_seq.AddPos.begin(pos)
    y = x
    for scale in (1.0, 2.0, 4.0):                               # three uses; their nodes receive 8 dy, 8 dy and 4 dy
        y = ops_seq.add_pos(y, pos) * scale
    y.backward(dy, retain_graph=True)
    assert len(seen) == 1 and torch.equal(seen[0], pos.grad)
    first = pos.grad.detach().clone()
    mag = 20.0 * dy.double().abs().sum(0).view(T, 1, D)          # sum of the magnitudes of the 3 B terms of one pass
    want = 20.0 * dy.double().sum(0).view(T, 1, D)
    assert bool(((first.double() - want).abs() <= 3 * B * U * mag).all())
    y.backward(dy)
    assert len(seen) == 2 and torch.equal(seen[1], pos.grad)
    # the second pass adds its 3 B terms one by one to what the first left: 6 B sequential additions over both
    assert bool(((pos.grad.double() - 2 * want).abs() <= 6 * B * U * 2 * mag).all())


def test_constant_embedding_passes_the_gradient_through(dev, monkeypatch):
    """the sine path: AddPos.backward hands dy itself on and launches nothing"""
    from buctd_amd import ops_seq

    def refuse(*a, **k):
        raise AssertionError("batch_sum launched for a constant embedding")

    monkeypatch.setattr(ops_seq, "batch_sum", refuse)
    x = torch.randn(B, T, D, device=dev, requires_grad=True)
    pos = torch.randn(T, D, device=dev)
    got = []
    x.register_hook(got.append)
    y = ops_seq.AddPos.apply(x, pos)
    assert torch.equal(y, x.detach() + pos)
    dy = torch.randn(B, T, D, device=dev)
    y.backward(dy)
    assert len(got) == 1 and got[0].data_ptr() == dy.data_ptr() and torch.equal(got[0], dy)
    assert not hasattr(pos, "_pos_uses")


# ---- the whole network through the engine ---------------------------------------------------------------------------------
def _cfg(pe, optimizer="adam"):
    from oracle import recipes
    c = recipes.CASES["transpose_w16_96x64"]()[0]
    c.MODEL.POS_EMBEDDING = pe
    c.TRAIN.OPTIMIZER = optimizer
    c.TRAIN.MOMENTUM, c.TRAIN.WD, c.TRAIN.NESTEROV = 0.9, 1e-4, False
    return c


def _net(cfg, dev, seed=11):
    from buctd_amd import models
    torch.manual_seed(seed)
    return models.transpose_h.get_pose_net(cfg, is_train=True).to(dev)


def _batch(cfg, n, seed, device):
    g = torch.Generator().manual_seed(seed)
    w, h = cfg.MODEL.IMAGE_SIZE
    hw, hh = cfg.MODEL.HEATMAP_SIZE
    k = cfg.MODEL.NUM_JOINTS
    x = torch.randn(n, 6, h, w, generator=g).to(device)
    t = torch.rand(n, k, hh, hw, generator=g).to(device)
    wt = (torch.rand(n, k, 1, generator=g) < 0.8).float().to(device)
    return x, t, wt


def _eager_step(model, opt, crit, x, t, w):
    from buctd_amd import ops
    ops.set_grad_arena(opt.flat)
    out = model(x)
    loss = crit(out, t, w)
    opt.zero_grad()
    loss.backward()
    opt.step()
    return out.detach().clone(), loss.detach().clone()


@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
def test_learnable_embedding_trains_through_the_engine(dev, optimizer):
    from buctd_amd import engine
    from buctd_amd.core.loss import JointsMSELoss
    cfg = _cfg("learnable", optimizer)
    net = _net(cfg, dev)
    tokens = (cfg.MODEL.IMAGE_SIZE[0] // 4) * (cfg.MODEL.IMAGE_SIZE[1] // 4)
    width = cfg.MODEL.DIM_MODEL + 16
    pe = net.pos_embedding
    assert pe.requires_grad and tuple(pe.shape) == (tokens, 1, width)
    model = engine.DataParallel(net)
    opt = engine.get_optimizer(cfg, model)
    assert isinstance(opt, engine.FusedAdam if optimizer == "adam" else engine.FusedSGD)
    assert net.pos_embedding is pe and opt.flat.owns(pe)          # the parameter lives in the arenas
    model.train()
    x, t, w = _batch(cfg, 2, 300, dev)
    before = pe.detach().clone()
    loss = JointsMSELoss(True)(model(x), t, w)
    opt.zero_grad()
    # dependency areas asked for between forward and backward: an eval forward under no_grad of the same encoder
    net.attention_maps(x, query=None)
    assert net.training
    loss.backward()
    assert opt.flat.grad_is_arena(pe) and tuple(pe.grad.shape) == (tokens, 1, width)
    gnorm = float(pe.grad.norm())
    assert gnorm > 0 and gnorm == gnorm
    opt.step()
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(pe).all())
    assert not torch.equal(pe.detach(), before)
    sd = net.state_dict()
    assert tuple(sd["pos_embedding"].shape) == (tokens, 1, width)
    fresh = _net(cfg, dev, seed=12)
    res = fresh.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    net.eval()
    fresh.eval()
    with torch.no_grad():
        assert torch.equal(net(x), fresh(x))


def test_network_without_an_embedding_trains_and_adds_none(dev, monkeypatch):
    from buctd_amd import engine, ops_seq
    from buctd_amd.core.loss import JointsMSELoss
    cfg = _cfg("none")
    net = _net(cfg, dev)
    assert net.pos_embedding is None and "pos_embedding" not in net.state_dict()
    calls = []
    real = ops_seq.add_bcast
    monkeypatch.setattr(ops_seq, "add_bcast", lambda *a: calls.append(1) or real(*a))
    model = engine.DataParallel(net)
    opt = engine.get_optimizer(cfg, model)
    model.train()
    x, t, w = _batch(cfg, 2, 301, dev)
    before = opt.flat.flat.clone()
    _, loss = _eager_step(model, opt, JointsMSELoss(True), x, t, w)
    assert bool(torch.isfinite(loss)) and not torch.equal(before, opt.flat.flat)
    assert not calls


def test_step_graph_replays_equal_eager_steps_bit_for_bit(dev):
    """the captured batch sums carry the accumulate flags of the capture: overwrite for the last layer's piece, accumulate for
    the others - what every eager step after zero_grad() does"""
    from buctd_amd import engine, ops
    from buctd_amd.core.loss import JointsMSELoss
    cfg = _cfg("learnable")
    net = _net(cfg, dev)
    pairs = []
    for i in range(2):
        model = engine.DataParallel(net if i == 0 else copy.deepcopy(net))
        opt = engine.get_optimizer(cfg, model)
        model.train()
        pairs.append((model, opt))
    (eager, eopt), (graphed, gopt) = pairs
    crit = JointsMSELoss(True)
    batches = [_batch(cfg, 2, 700 + i, dev) for i in range(5)]
    ops.manual_seed(0x5EED)
    ref = []
    for b in batches:
        out, loss = _eager_step(eager, eopt, crit, *b)
        ref.append((out, loss, eopt.flat.grad.clone()))
    drawn = ops.seeds_drawn()
    ops.manual_seed(0x5EED)
    ops.set_grad_arena(gopt.flat)
    step = engine.StepGraph(graphed, crit, gopt, warmup=2, fresh_dropout_masks=True)
    for i, b in enumerate(batches):
        ops.set_grad_arena(gopt.flat)
        out, loss = step(*b)
        assert torch.equal(loss.detach(), ref[i][1]), (i, float(loss), float(ref[i][1]))
        assert torch.equal(out.detach(), ref[i][0]), i
        assert torch.equal(gopt.flat.grad, ref[i][2]), i
    assert step.replays == 3 and ops.seeds_drawn() == drawn
    assert float(graphed.module.pos_embedding.grad.norm()) > 0
    assert torch.equal(eopt.flat.flat, gopt.flat.flat)
    assert torch.equal(eopt.exp_avg, gopt.exp_avg) and torch.equal(eopt.exp_avg_sq, gopt.exp_avg_sq)
    sd_e, sd_g = eager.module.state_dict(), graphed.module.state_dict()
    for k in sd_e:
        assert torch.equal(sd_e[k], sd_g[k]), k


def test_forward_graph_notices_the_optimizer_rewriting_the_embedding(dev):
    from buctd_amd import engine
    from buctd_amd.core.loss import JointsMSELoss
    cfg = _cfg("learnable")
    net = _net(cfg, dev)
    model = engine.DataParallel(net)
    opt = engine.get_optimizer(cfg, model)
    fg = engine.ForwardGraph(net, warmup=1, autoselect=False)
    x, t, w = _batch(cfg, 2, 900, dev)
    net.eval()
    with torch.no_grad():
        for _ in range(3):
            assert torch.equal(fg(x), net(x))
    assert fg.replays == 2
    old = net.pos_embedding.detach().clone()
    net.train()
    _eager_step(model, opt, JointsMSELoss(True), x, t, w)
    net.eval()
    assert not torch.equal(old, net.pos_embedding.detach())
    with torch.no_grad():
        want = net(x)
        for _ in range(3):
            assert torch.equal(fg(x), want)
    assert fg.replays == 4
