"""The host skeleton of engine.FusedAdam / FusedSGD, without a device: what a step() calls and in which order for the plain
and the grouped form with the norm clip off and on (the launchers are replaced by recorders), the checkpoint formats in both
directions with every refusal of load_state_dict, and the span arithmetic of FlatParams."""
import copy

import pytest
import torch

from tests.helpers import param_groups_ref as R

# the arena of small_net(): six slots, each padded to a multiple of four floats
SLOTS = [(0, 164), (164, 172), (172, 180), (180, 188), (188, 208), (208, 212)]
NUMEL = 212
EPS = 2.0 ** -10          # every hyper-parameter below is a binary fraction: it reads back exactly from the fp32 group tables
GSCALE, MAX_NORM = 0.5, 2.0


def small_net():
    """three layers whose parameter sizes (162, 6, 6, 6, 18, 3) are no multiples of the arena's alignment"""
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Conv2d(3, 6, 3), torch.nn.BatchNorm2d(6), torch.nn.Conv2d(6, 3, 1))


# ---- step trace ---------------------------------------------------------------------------------------------------------------
class Recorder:
    """replaces the launchers of buctd_amd.ops by functions that note their name and their plain-Python arguments"""

    def __init__(self, monkeypatch):
        from buctd_amd import _C, ops
        self.calls = []
        self.table = torch.zeros(16, dtype=torch.uint8)
        note = self.calls.append
        runs_of = lambda runs: [tuple(r) for r in runs]      # noqa: E731

        def adam_step(p, g, m, v, lr, b1, b2, eps, step, gscale=1.0, coef=None):
            note(("adam_step", p.numel(), lr, b1, b2, eps, step, gscale, coef is None))

        def sgd_step(p, g, buf, lr, momentum, wd, nesterov, first, gscale=1.0, coef=None):
            run = (p.storage_offset(), p.storage_offset() + p.numel())
            assert g.storage_offset() == run[0] and (buf is None or buf.storage_offset() == run[0])
            note(("sgd_step", run, buf is None, lr, momentum, wd, nesterov, first, gscale, coef is None))

        def adam_step_groups(p, g, m, v, table, groups, gscale=1.0, coef=None):
            assert table is self.table and isinstance(groups, _C.AdamGroup * len(groups))
            note(("adam_step_groups", [(t.lr, t.beta1, t.beta2, t.eps, t.weight_decay, t.decoupled, t.step) for t in groups],
                  gscale, coef is None))

        def sgd_step_groups(p, g, buf, table, groups, gscale=1.0, coef=None):
            assert table is self.table and isinstance(groups, _C.SgdGroup * len(groups))
            note(("sgd_step_groups", buf is None, [(t.lr, t.momentum, t.weight_decay, t.nesterov) for t in groups], gscale,
                  coef is None))

        def step_chunks(runs, owners, numel):
            note(("step_chunks", runs_of(runs), list(owners), numel))
            return "chunks"

        def step_chunk_table(chunks, device):
            assert chunks == "chunks"
            note(("step_chunk_table",))
            return self.table

        def grad_sumsq_workspace(runs):
            note(("grad_sumsq_workspace", runs_of(runs)))
            return 8

        def grad_sumsq(g, runs, out, workspace):
            note(("grad_sumsq", runs_of(runs)))

        def grad_clip_coef(sumsq, gscale, max_norm, coef, norm):
            note(("grad_clip_coef", gscale, max_norm))

        def weights_updated(_real=ops.weights_updated):
            note(("weights_updated",))
            _real()

        def refresh_prepared(device):
            note(("refresh_prepared",))

        for f in (adam_step, sgd_step, adam_step_groups, sgd_step_groups, step_chunks, step_chunk_table, grad_sumsq_workspace,
                  grad_sumsq, grad_clip_coef, weights_updated, refresh_prepared):
            monkeypatch.setattr(ops, f.__name__, f)

    def grad_sync(self):
        self.calls.append(("grad_sync",))
        return GSCALE

    def update(self):              # the stub of optimizer.avg
        self.calls.append(("avg.update",))

    def watch_collect(self, flat, monkeypatch):
        def collect(_real=flat.collect):
            self.calls.append(("collect",))
            _real()
        monkeypatch.setattr(flat, "collect", collect)

    def take(self):
        out, self.calls[:] = list(self.calls), []
        return out


def make(kind, grouped, rec, clip):
    from buctd_amd import engine
    flat = engine.FlatParams(small_net())
    ps = flat.params
    kw = dict(grad_sync=rec.grad_sync, max_grad_norm=MAX_NORM if clip else None)
    if kind == "adam":
        groups = [{"params": ps[:2], "lr": 0.5}, {"params": ps[2:4], "lr": 0.25, "weight_decay": 0.25},
                  {"params": ps[4:], "lr": 0.125, "betas": (0.25, 0.5)}]
        return engine.FusedAdam(flat, lr=0.5, betas=(0.5, 0.75), eps=EPS, groups=groups if grouped else None, **kw)
    if grouped:
        groups = [{"params": ps[:2], "lr": 0.5, "momentum": 0.5, "weight_decay": 0.25, "nesterov": True},
                  {"params": ps[2:4], "lr": 0.25}, {"params": ps[4:], "lr": 0.125, "momentum": 0.25}]
        return engine.FusedSGD(flat, lr=1.0, groups=groups, **kw)
    return engine.FusedSGD(flat, lr=0.5, momentum=0.5, weight_decay=0.25, nesterov=True, **kw)


HEAD = [("collect",), ("grad_sync",)]
TAIL = [("weights_updated",), ("refresh_prepared",)]
AVG = [("avg.update",)]
ALL, ONE = [(0, NUMEL)], [SLOTS[4]]


def measured(clip, runs):
    """what the norm clip enqueues in front of the launch: the reduction over the runs (none: nothing to reduce), the finalize"""
    if not clip:
        return []
    return ([("grad_sumsq_workspace", runs), ("grad_sumsq", runs)] if runs else []) + [("grad_clip_coef", GSCALE, MAX_NORM)]


def adam_table(steps):
    return [(0.5, 0.5, 0.75, EPS, 0.0, 0, steps[0]), (0.25, 0.5, 0.75, EPS, 0.25, 0, steps[1]),
            (0.125, 0.25, 0.5, EPS, 0.0, 0, steps[2])]


SGD_TABLE = [(0.5, 0.5, 0.25, 1), (0.25, 0.0, 0.0, 0), (0.125, 0.25, 0.0, 0)]
BUILD_ALL = [("step_chunks", [(0, 172), (172, 188), (188, 212)], [0, 1, 2], NUMEL), ("step_chunk_table",)]
BUILD_ONE = [("step_chunks", ONE, [2], NUMEL), ("step_chunk_table",)]


def expected(kind, grouped, clip):
    """the calls of three steps - a gradient on every parameter, on parameter 4 alone, on none - and, after each step,
    (step_count, group_steps, table_builds, zeroed, weights_epoch delta)"""
    off = not clip
    if kind == "adam" and not grouped:          # one launch over the whole arena whatever holds a gradient
        calls = [HEAD + measured(clip, runs) + [("adam_step", NUMEL, 0.5, 0.5, 0.75, EPS, k, GSCALE, off)] + TAIL + AVG
                 for k, runs in ((1, ALL), (2, ONE), (3, []))]
        return calls, [(1, None, None, 1, 1), (2, None, None, 2, 1), (3, None, None, 3, 1)]
    if kind == "sgd" and not grouped:           # one launch per gradient run; the tail runs without a launch too
        launch = lambda run: ("sgd_step", run, False, 0.5, 0.5, 0.25, True, False, GSCALE, off)      # noqa: E731
        calls = [HEAD + measured(clip, runs) + [launch(r) for r in runs] + TAIL + AVG for runs in (ALL, ONE, [])]
        return calls, [(1, None, None, 1, 1), (2, None, None, 2, 1), (3, None, None, 3, 1)]
    if kind == "adam":
        launch = lambda steps: [("adam_step_groups", adam_table(steps), GSCALE, off)]      # noqa: E731
        calls = [HEAD + BUILD_ALL + measured(clip, ALL) + launch([1, 1, 1]) + TAIL + AVG,
                 HEAD + BUILD_ONE + measured(clip, ONE) + launch([1, 1, 2]) + TAIL + AVG,
                 HEAD + measured(clip, []) + AVG]          # no live gradient: measured, counted, no launch and no tail
        return calls, [(1, [1, 1, 1], 1, 1, 1), (2, [1, 1, 2], 2, 2, 1), (3, [1, 1, 2], 2, 3, 0)]
    launch = [("sgd_step_groups", False, SGD_TABLE, GSCALE, off)]
    calls = [HEAD + BUILD_ALL + measured(clip, ALL) + launch + TAIL + AVG,
             HEAD + BUILD_ONE + measured(clip, ONE) + launch + TAIL + AVG,
             HEAD + measured(clip, []) + AVG]
    return calls, [(1, None, 1, 1, 1), (2, None, 2, 2, 1), (3, None, 2, 3, 0)]


@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "grouped"])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_step_trace(kind, grouped, clip, monkeypatch):
    from buctd_amd import ops
    rec = Recorder(monkeypatch)
    opt = make(kind, grouped, rec, clip)
    rec.watch_collect(opt.flat, monkeypatch)
    opt.avg = rec
    assert getattr(opt, "zeroed", 0) == 0 and opt.step_count == 0 and opt.grouped == grouped
    assert opt.flat.optimizer() is opt and opt.last_grad_norm is None and opt.last_clip_coef is None
    assert [opt.flat.offsets[id(p)] for p in opt.flat.params] == [s for s, _ in SLOTS] and opt.flat.numel == NUMEL
    want_calls, want_counts = expected(kind, grouped, clip)
    gen = torch.Generator().manual_seed(1)
    for k, live in enumerate((range(6), [4], [])):
        opt.zero_grad()
        assert all(p.grad is None for p in opt.flat.params)
        for i in live:
            p = opt.flat.params[i]
            p.grad = torch.randn(p.shape, generator=gen)
        epoch = ops.weights_epoch()
        opt.step()
        assert rec.take() == want_calls[k], f"step {k + 1}"
        got = (opt.step_count, getattr(opt, "group_steps", None), getattr(opt, "table_builds", None), opt.zeroed,
               ops.weights_epoch() - epoch)
        assert got == want_counts[k], f"step {k + 1}"
        assert (opt.last_grad_norm is None) == (not clip) and (opt.last_clip_coef is None) == (not clip)
    with pytest.raises(NotImplementedError, match="closures"):
        opt.step(lambda: 0.0)
    assert rec.take() == []
    opt.max_grad_norm = -1.0
    with pytest.raises(ValueError, match="max_grad_norm must be positive"):
        opt.step()


# ---- checkpoints --------------------------------------------------------------------------------------------------------------
def torch_sd(cls, net, groups=None, late=(), steps=2, **kw):
    """the state_dict of torch's optimizer over the parameters of `net` after `steps` CPU steps; the parameters `late` join at
    the second step"""
    ps = list(net.parameters())
    ref = cls(ps if groups is None else [dict(g, params=[ps[i] for i in g["params"]]) for g in groups], **kw)
    gen = torch.Generator().manual_seed(3)
    for k in range(steps):
        for i, p in enumerate(ps):
            p.grad = None if (k == 0 and i in late) else torch.randn(p.shape, generator=gen)
        ref.step()
    return ref.state_dict()


TWO = [{"params": [0, 1, 2]}, {"params": [3, 4, 5]}]


def fused(kind, groups=None, **kw):
    from buctd_amd import engine
    flat = engine.FlatParams(small_net())
    if groups is not None:
        kw["groups"] = [dict(g, params=[flat.params[i] for i in g["params"]]) for g in groups]
    return (engine.FusedAdam if kind == "adam" else engine.FusedSGD)(flat, **kw)


def same_state(out, sd):
    assert out["state"].keys() == sd["state"].keys()
    for i, st in sd["state"].items():
        assert out["state"][i].keys() == st.keys()
        for k, v in st.items():
            assert torch.equal(out["state"][i][k], v) if torch.is_tensor(v) else out["state"][i][k] == v, (i, k)


@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_plain_sgd_checkpoint_is_torch_sgd_format(momentum):
    sd = torch_sd(torch.optim.SGD, small_net(), lr=0.05, momentum=momentum, weight_decay=1e-4, nesterov=momentum > 0)
    opt = fused("sgd", lr=0.01, momentum=momentum)
    fresh = opt.state_dict()
    assert fresh["state"] == {} and fresh["param_groups"][0].keys() == sd["param_groups"][0].keys()
    opt.load_state_dict(copy.deepcopy(sd))
    assert opt.step_count == (1 if momentum else 0) and (opt.buf is None) == (momentum == 0)
    out = opt.state_dict()
    assert out["param_groups"] == sd["param_groups"] and out["param_groups"][0]["params"] == list(range(6))
    assert len(out["state"]) == (6 if momentum else 0)
    same_state(out, sd)
    strs = dict(sd, state={str(i): st for i, st in sd["state"].items()})      # as a JSON-like store returns the keys
    again = fused("sgd", lr=0.01, momentum=momentum)
    again.load_state_dict(strs)
    same_state(again.state_dict(), sd)


def test_plain_adam_state_dict_keys_and_the_old_flat_format():
    opt = fused("adam", lr=0.5, betas=(0.5, 0.75), eps=EPS)
    fresh = opt.state_dict()
    assert fresh["state"] == {}, "no state before the first step"
    assert fresh["param_groups"] == [{"lr": 0.5, "betas": (0.5, 0.75), "eps": EPS, "weight_decay": 0, "amsgrad": False,
                                      "maximize": False, "params": list(range(6))}]
    gen = torch.Generator().manual_seed(4)
    old = {"step": 7, "exp_avg": torch.randn(NUMEL, generator=gen), "exp_avg_sq": torch.rand(NUMEL, generator=gen),
           "param_groups": [{"lr": 0.25, "betas": (0.5, 0.5), "eps": EPS, "params": list(range(6))}]}
    opt.load_state_dict(copy.deepcopy(old))
    assert opt.step_count == 7 and opt.param_groups[0]["lr"] == 0.25 and opt.param_groups[0]["betas"] == (0.5, 0.5)
    assert torch.equal(opt.exp_avg, old["exp_avg"]) and torch.equal(opt.exp_avg_sq, old["exp_avg_sq"])
    out = opt.state_dict()
    assert sorted(out["state"]) == list(range(6))
    for i, (p, (s, _)) in enumerate(zip(opt.flat.params, SLOTS)):
        st = out["state"][i]
        assert st.keys() == {"step", "exp_avg", "exp_avg_sq"} and float(st["step"]) == 7.0
        for name in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(st[name], torch.as_strided(old[name], p.shape, p.stride(), s))
    # torch's format back in, under string keys
    sd = torch_sd(torch.optim.Adam, small_net(), lr=1e-3)
    opt.load_state_dict(dict(sd, state={str(i): st for i, st in sd["state"].items()}))
    assert opt.step_count == 2
    same_state(opt.state_dict(), sd)


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_grouped_state_dict_fills_the_torch_defaults(kind):
    if kind == "sgd":
        opt, want = fused("sgd", TWO, lr=0.1), torch.optim.SGD([torch.zeros(1)], lr=0.1).defaults
    else:
        opt, want = fused("adam", TWO, lr=0.1), torch.optim.Adam([torch.zeros(1)], lr=0.1).defaults
    sd = opt.state_dict()
    assert sd["state"] == {} and [g["params"] for g in sd["param_groups"]] == [[0, 1, 2], [3, 4, 5]]
    for g in sd["param_groups"]:
        assert set(want) <= g.keys() and "max_grad_norm" not in g
    decoupled = fused("adam", TWO, lr=0.1, decoupled_weight_decay=True).state_dict()
    assert decoupled["param_groups"][0].keys() >= set(torch.optim.AdamW([torch.zeros(1)], lr=0.1).defaults)


def test_grouped_sgd_load_allocates_the_buffer_and_writes_no_state_without_momentum():
    groups = [dict(TWO[0], momentum=0.9), dict(TWO[1], momentum=0.0)]
    sd = torch_sd(torch.optim.SGD, small_net(), groups, lr=0.05)
    opt = fused("sgd", TWO, lr=0.05, momentum=0.5)
    opt.load_state_dict(copy.deepcopy(sd))
    assert opt.step_count == 1 and [g["momentum"] for g in opt.param_groups] == [0.9, 0.0]
    out = opt.state_dict()
    assert sorted(out["state"]) == [0, 1, 2], "no state for the group without momentum"
    same_state(out, sd)
    # a checkpoint from before the first step brings a momentum and no buffers: the arena for them is made on load
    empty = fused("sgd", TWO, lr=0.05)
    assert empty.buf is None
    empty.load_state_dict(torch_sd(torch.optim.SGD, small_net(), groups, steps=0, lr=0.05))
    assert empty.buf is not None and not empty.buf.any() and empty.step_count == 0 and empty.state_dict()["state"] == {}


def bad_adam(edit=None, **kw):
    sd = torch_sd(torch.optim.Adam, small_net(), lr=1e-3, **kw)
    if edit:
        edit(sd)
    return sd


def set_group(key, value, gi=0):
    return lambda sd: sd["param_groups"][gi].__setitem__(key, value)


def wrong_shape(sd):
    sd["state"][0]["exp_avg"] = torch.zeros(2)


REFUSALS = {
    "adam_plain_weight_decay": lambda: (fused("adam"), bad_adam(weight_decay=0.1), "implements Adam without weight decay"),
    "adam_plain_amsgrad": lambda: (fused("adam"), bad_adam(set_group("amsgrad", True)), "FusedAdam does not implement amsgrad"),
    "adam_plain_maximize": lambda: (fused("adam"), bad_adam(set_group("maximize", True)),
                                    "FusedAdam does not implement maximize"),
    "adam_plain_steps_differ": lambda: (fused("adam"), bad_adam(late=[2]),
                                        "keeps one step counter: per-parameter steps differ in this state_dict"),
    "adam_plain_shape": lambda: (fused("adam"), bad_adam(wrong_shape), r"optimizer state of parameter 0: shape \(2,\) != \(6, 3, 3, 3\)"),
    "adam_grouped_steps_differ": lambda: (fused("adam", TWO), bad_adam(groups=TWO, late=[2]),
                                          r"one step counter per group: the steps of group 0 differ in this state_dict \(\[1, 2\]\)"),
    "adam_grouped_shape": lambda: (fused("adam", TWO), bad_adam(wrong_shape, groups=TWO),
                                   r"optimizer state of parameter '0\.weight': shape \(2,\) != \(6, 3, 3, 3\)"),
    "adam_grouped_amsgrad": lambda: (fused("adam", TWO), bad_adam(set_group("amsgrad", True, 1), groups=TWO),
                                     "FusedAdam does not implement amsgrad"),
    "adam_grouped_maximize": lambda: (fused("adam", TWO), bad_adam(set_group("maximize", True, 1), groups=TWO),
                                      "FusedAdam does not implement maximize"),
    "adam_group_count": lambda: (fused("adam", TWO), bad_adam(), "the state_dict has 1 parameter groups, this optimizer 2"),
    "adam_parameter_count": lambda: (fused("adam", TWO), bad_adam(groups=[{"params": [0, 1]}, {"params": [2, 3, 4, 5]}]),
                                     "group 0 of the state_dict has 2 parameters, this optimizer's 3"),
    "sgd_plain_dampening": lambda: (fused("sgd", momentum=0.9),
                                    torch_sd(torch.optim.SGD, small_net(), lr=0.1, momentum=0.9, dampening=0.5),
                                    r"FusedSGD implements dampening = 0 \(the reference's recipe\)"),
    "sgd_plain_maximize": lambda: (fused("sgd"), torch_sd(torch.optim.SGD, small_net(), lr=0.1, maximize=True),
                                   "FusedSGD does not implement maximize"),
    "sgd_plain_buffers_without_momentum": lambda: (fused("sgd"), torch_sd(torch.optim.SGD, small_net(), lr=0.1, momentum=0.9),
                                                   "built without momentum but the state_dict carries momentum buffers"),
    "sgd_grouped_dampening": lambda: (fused("sgd", TWO, momentum=0.9),
                                      torch_sd(torch.optim.SGD, small_net(), TWO, lr=0.1, momentum=0.9, dampening=0.5),
                                      r"FusedSGD implements dampening = 0 \(the reference's recipe\)"),
    "sgd_grouped_maximize": lambda: (fused("sgd", TWO), torch_sd(torch.optim.SGD, small_net(), TWO, lr=0.1, maximize=True),
                                     "FusedSGD does not implement maximize"),
    "sgd_grouped_buffers_without_momentum": lambda: (fused("sgd", TWO),
                                                     torch_sd(torch.optim.SGD, small_net(), TWO, lr=0.1, momentum=0.9),
                                                     "built without momentum but the state_dict carries momentum buffers"),
    "sgd_group_count": lambda: (fused("sgd", TWO), torch_sd(torch.optim.SGD, small_net(), lr=0.1),
                                "the state_dict has 1 parameter groups, this optimizer 2"),
    "sgd_parameter_count": lambda: (fused("sgd", TWO),
                                    torch_sd(torch.optim.SGD, small_net(), [{"params": [0]}, {"params": [1, 2, 3, 4, 5]}], lr=0.1),
                                    "group 0 of the state_dict has 1 parameters, this optimizer's 3"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_load_state_dict_refuses(case):
    opt, sd, message = REFUSALS[case]()
    with pytest.raises(ValueError, match=message):
        opt.load_state_dict(sd)


# ---- spans --------------------------------------------------------------------------------------------------------------------
def runs_as_the_loops_merged_them(spans, keys=None):
    """the merging loop the engine carried three times before FlatParams.merge_spans, restated"""
    runs, out = [], []
    for i, (s, e) in enumerate(spans):
        k = None if keys is None else keys[i]
        if runs and runs[-1][1] == s and out[-1] == k:
            runs[-1][1] = e
        else:
            runs.append([s, e])
            out.append(k)
    return [(s, e) for s, e in runs], out


class Lengths(torch.nn.Module):
    def __init__(self, lengths):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.zeros(n)) for n in lengths])


def test_grad_runs_cover_the_padded_slots_of_the_parameters_that_hold_a_gradient():
    from buctd_amd import engine
    lengths = [n - d for n, d in zip(R.SPAN_LENGTHS, (0, 1, 2, 3, 5))] + [1, 7]
    flat = engine.FlatParams(Lengths(lengths))
    up = lambda n: (n + 3) // 4 * 4      # noqa: E731
    starts = [sum(up(n) for n in lengths[:i]) for i in range(len(lengths))]
    assert [flat.offsets[id(p)] for p in flat.params] == starts and flat.numel == starts[-1] + 8
    assert [flat.span(p) for p in flat.params] == [(s, s + n) for s, n in zip(starts, lengths)]
    assert flat.grad_runs() == []
    for live, want in (([0, 1, 2, 3, 4, 5, 6], [(0, flat.numel)]),
                       ([1, 2, 4, 6], [(starts[1], starts[3]), (starts[4], starts[5]), (starts[6], flat.numel)]),
                       ([3], [(starts[3], starts[4])])):
        for i, p in enumerate(flat.params):
            p.grad = torch.zeros_like(p) if i in live else None
        assert flat.grad_runs() == want
        assert all(s % 4 == 0 and e % 4 == 0 for s, e in flat.grad_runs())


def test_aligned_span_and_merge_spans():
    from buctd_amd import engine
    flat = engine.FlatParams(small_net())
    assert [flat.aligned_span(p) for p in flat.params] == SLOTS
    merge = engine.FlatParams.merge_spans
    gapped, _ = R.layout(R.SPAN_LENGTHS)                     # gaps of 4 and 8 elements: nothing to merge
    assert merge(gapped) == (gapped, [None] * len(gapped))
    packed, at = [], 8
    for n in R.SPAN_LENGTHS + R.SPAN_LENGTHS:                # back to back, one gap in the middle
        at += 8 if len(packed) == len(R.SPAN_LENGTHS) else 0
        packed.append((at, at + n))
        at += n
    assert merge(packed) == runs_as_the_loops_merged_them(packed)
    assert merge(packed)[0] == [(8, packed[4][1]), (packed[5][0], at)]
    keys = [0, 0, 1, 1, 1, 1, 2, 0, 0, 0]
    runs, owners = merge(packed, keys)                       # with keys: broken where the key changes, and at the gap
    assert (runs, owners) == runs_as_the_loops_merged_them(packed, keys)
    assert owners == [0, 1, 1, 2, 0]
    assert runs == [(8, packed[1][1]), (packed[2][0], packed[4][1]), (packed[5][0], packed[5][1]), (packed[6][0], packed[6][1]),
                    (packed[7][0], at)]
    assert merge([]) == ([], []) and merge(SLOTS)[0] == [(0, NUMEL)]
