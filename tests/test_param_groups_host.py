"""Parameter groups on the flat arena, the parts that need no device: the chunk table (buctd_step_chunks), construction
errors of the grouped FusedAdam / FusedSGD, state dicts in torch's format in both directions, schedulers, groups_by_name
and get_last_layer_optimizer (reference lib/utils/utils.py:277-290)."""
import copy
import ctypes as C

import pytest
import torch

from tests.helpers import param_groups_ref as R


def small_net():
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3), torch.nn.BatchNorm2d(8), torch.nn.Conv2d(8, 4, 1))
    return net


def chunks_of(runs, owners, out=True):
    from buctd_amd import _C
    arr = (C.c_long * (2 * len(runs)))(*[v for r in runs for v in r])
    grp = (C.c_int * len(owners))(*owners)
    n = _C.lib().buctd_step_chunks(arr, grp, len(runs), None)
    if n < 0 or not out:
        return n
    buf = (_C.StepChunk * n)()
    assert _C.lib().buctd_step_chunks(arr, grp, len(runs), buf) == n, "the count-only call and the filling call disagree"
    return [(c.start, c.len, c.group) for c in buf]


def test_header_constants_are_bound():
    from buctd_amd import _C
    assert (_C.STEP_MAX_GROUPS, _C.STEP_CHUNK) == (R.MAX_GROUPS, R.CHUNK) and C.sizeof(_C.StepChunk) == 16
    assert C.sizeof(_C.AdamGroup) == 28 and C.sizeof(_C.SgdGroup) == 16


@pytest.mark.parametrize("n", R.SPAN_LENGTHS)
def test_step_chunks_split_one_run(n):
    got = chunks_of([(8, 8 + n)], [3])
    assert got == R.expected_chunks([(8, 8 + n)], [3])
    assert len(got) == (n + R.CHUNK - 1) // R.CHUNK and sum(c[1] for c in got) == n
    assert all(0 < c[1] <= R.CHUNK and c[1] % 4 == 0 and c[0] % 4 == 0 and c[2] == 3 for c in got)


def test_step_chunks_tile_the_runs_in_order():
    spans, _ = R.layout(R.SPAN_LENGTHS + R.SPAN_LENGTHS)
    owners = [k % 5 for k in range(len(spans))]
    got = chunks_of(spans, owners)
    assert got == R.expected_chunks(spans, owners)
    at = 0
    for (s, e), g in zip(spans, owners):        # the chunks of a run follow each other from its start to its end
        pos = s
        while pos < e:
            assert got[at][0] == pos and got[at][2] == g
            pos += got[at][1]
            at += 1
        assert pos == e
    assert at == len(got)
    # adjacent runs of different groups stay apart
    assert chunks_of([(0, 8), (8, 16)], [0, 1]) == [(0, 8, 0), (8, 8, 1)]


@pytest.mark.parametrize("runs, owners", [
    ([(2, 10)], [0]), ([(0, 10)], [0]),                     # unaligned start, unaligned end
    ([(0, 16), (12, 32)], [0, 1]), ([(16, 32), (0, 8)], [0, 0]),   # overlapping, descending
    ([(8, 8)], [0]), ([(12, 8)], [0]),                      # empty
    ([(0, 8)], [16]), ([(0, 8)], [-1]),                     # group id outside [0, 16)
])
def test_step_chunks_refuses(runs, owners):
    from buctd_amd import _C
    assert chunks_of(runs, owners, out=False) == -1
    assert b"buctd_step_chunks" in _C.lib().buctd_last_error()
    from buctd_amd import ops
    with pytest.raises(_C.BuctdHipError):
        ops.step_chunks(runs, owners, 1 << 20)


def test_ops_step_chunks_refuses_a_run_behind_the_arena():
    from buctd_amd import _C, ops
    assert len(ops.step_chunks([(0, 64)], [0], 64)) == 1
    with pytest.raises(_C.BuctdHipError):
        ops.step_chunks([(0, 64)], [0], 60)


@pytest.mark.parametrize("cls", ["adam", "sgd"])
def test_construction_errors(cls):
    from buctd_amd import engine
    make = engine.FusedAdam if cls == "adam" else engine.FusedSGD
    net = small_net()
    flat = engine.FlatParams(net)
    ps = list(net.parameters())
    with pytest.raises(ValueError, match="not in the arena"):
        make(flat, groups=[{"params": [torch.nn.Parameter(torch.zeros(5, 3))]}])
    with pytest.raises(ValueError, match=r"'0\.bias'.*group 0.*group 1"):
        make(flat, groups=[{"params": ps[:2]}, {"params": ps[1:3]}])
    with pytest.raises(ValueError, match="17 parameter groups"):
        make(flat, groups=[{"params": []} for _ in range(17)])
    make(flat, groups=[{"params": []} for _ in range(15)] + [{"params": ps}])      # 16 are possible
    sync = lambda: 1.0      # noqa: E731
    with pytest.raises(ValueError, match=r"'2\.bias' is in no group"):
        make(flat, groups=[{"params": ps[:-1]}], grad_sync=sync)
    ps[0].requires_grad = False
    with pytest.raises(ValueError, match=r"'0\.weight' is frozen"):
        make(flat, groups=[{"params": ps}], grad_sync=sync)
    ps[0].requires_grad = True
    opt = make(flat, groups=[{"params": ps[:3], "lr": 0.5}, {"params": ps[3:]}], grad_sync=sync)
    assert opt.grouped and opt.param_groups[0]["lr"] == 0.5 and len(opt.param_groups) == 2


def three_groups(ps, kind):
    if kind == "sgd":
        return [{"params": ps[:2], "lr": 0.1, "momentum": 0.9, "weight_decay": 1e-4, "nesterov": True},
                {"params": ps[2:4], "lr": 0.01, "momentum": 0.5},
                {"params": ps[4:], "lr": 0.2, "momentum": 0.9, "weight_decay": 1e-2}]
    return [{"params": ps[:2], "lr": 1e-2, "betas": (0.8, 0.99)},
            {"params": ps[2:4], "lr": 1e-3, "weight_decay": 1e-2, "eps": 1e-6},
            {"params": ps[4:], "lr": 5e-4, "weight_decay": 1e-1}]


def make_torch(kind, groups):
    if kind == "sgd":
        return torch.optim.SGD(groups, lr=1.0)
    return (torch.optim.AdamW if kind == "adamw" else torch.optim.Adam)(groups, lr=1.0, weight_decay=0.0)


def make_fused(kind, flat, groups):
    from buctd_amd import engine
    if kind == "sgd":
        return engine.FusedSGD(flat, lr=1.0, groups=groups)
    return engine.FusedAdam(flat, lr=1.0, groups=groups, decoupled_weight_decay=kind == "adamw")


@pytest.mark.parametrize("kind", ["adam", "adamw", "sgd"])
def test_state_dict_round_trips_with_torch(kind):
    """torch -> fused -> torch with three groups whose parameters stepped 3, 2 and 0 times; then the fused optimizer's own
    state_dict is loaded by a fresh torch optimizer, which steps on with it"""
    from buctd_amd import engine
    net = small_net()
    twin = copy.deepcopy(net)
    ps = list(net.parameters())
    ref = make_torch(kind, three_groups(ps, kind))
    for k in range(3):
        ref.zero_grad()
        for p in ps[:2] + (ps[2:4] if k else []):       # group 1 joins at the second step, group 2 never
            p.grad = torch.randn_like(p)
        ref.step()
    sd = ref.state_dict()
    flat = engine.FlatParams(twin)
    fused = make_fused(kind, flat, three_groups(flat.params, kind))
    fused.load_state_dict(copy.deepcopy(sd))
    if kind != "sgd":
        assert fused.group_steps == [3, 2, 0]
    for g, src in zip(fused.param_groups, sd["param_groups"]):
        assert all(g[k] == src[k] for k in ("lr", "weight_decay"))
    out = fused.state_dict()
    assert sorted(out["state"]) == sorted(sd["state"]) == [0, 1, 2, 3]
    assert [g["params"] for g in out["param_groups"]] == [g["params"] for g in sd["param_groups"]] == [[0, 1], [2, 3], [4, 5]]
    for i, st in sd["state"].items():
        for k, v in st.items():
            assert torch.equal(out["state"][i][k], v) if torch.is_tensor(v) else out["state"][i][k] == v, (i, k)
    back = make_torch(kind, three_groups(list(copy.deepcopy(net).parameters()), kind))
    back.load_state_dict(out)
    for g, src in zip(back.param_groups, sd["param_groups"]):
        assert {k: v for k, v in g.items() if k != "params"} == {k: v for k, v in src.items() if k != "params"}
    for p in back.param_groups[0]["params"] + back.param_groups[2]["params"]:
        p.grad = torch.ones_like(p)
    back.step()                                        # torch finds every key it reads in what the fused optimizer wrote
    if kind != "sgd":
        assert float(back.state[back.param_groups[0]["params"][0]]["step"]) == 4.0
        assert float(back.state[back.param_groups[2]["params"][0]]["step"]) == 1.0


def test_differing_steps_inside_a_group_are_refused():
    from buctd_amd import engine
    net = small_net()
    ps = list(net.parameters())
    ref = torch.optim.Adam([{"params": ps[:3]}, {"params": ps[3:]}], lr=1e-3)
    for k in range(2):
        for p in ps[:2] + (ps[2:] if k else []):       # ps[2] joins its group a step late
            p.grad = torch.randn_like(p)
        ref.step()
    flat = engine.FlatParams(copy.deepcopy(net))
    fused = engine.FusedAdam(flat, groups=[{"params": flat.params[:3]}, {"params": flat.params[3:]}])
    with pytest.raises(ValueError, match="group 0 differ"):
        fused.load_state_dict(ref.state_dict())
    with pytest.raises(ValueError, match="parameter groups"):
        engine.FusedAdam(flat, groups=[{"params": flat.params}]).load_state_dict(ref.state_dict())
    for key in ("amsgrad", "maximize"):
        bad = copy.deepcopy(torch.optim.Adam([{"params": ps[:3]}, {"params": ps[3:]}]).state_dict())
        bad["param_groups"][1][key] = True
        with pytest.raises(ValueError, match=key):
            fused.load_state_dict(bad)
    sgd = engine.FusedSGD(flat, groups=[{"params": flat.params, "momentum": 0.9}])
    bad = torch.optim.SGD(ps, lr=0.1, momentum=0.9, dampening=0.5).state_dict()
    with pytest.raises(ValueError, match="dampening"):
        sgd.load_state_dict(bad)
    with pytest.raises(ValueError, match="dampening"):
        engine.FusedSGD(flat, groups=[{"params": flat.params, "dampening": 0.1}])


def test_plain_fused_adam_is_unchanged_and_still_refuses_weight_decay():
    from buctd_amd import engine
    net = small_net()
    flat = engine.FlatParams(net)
    plain = engine.FusedAdam(flat, lr=1e-3)
    assert not plain.grouped and len(plain.param_groups) == 1 and "weight_decay" not in plain.param_groups[0]
    sd = torch.optim.Adam(list(copy.deepcopy(net).parameters()), lr=1e-3, weight_decay=0.1).state_dict()
    with pytest.raises(ValueError):
        plain.load_state_dict(sd)
    assert not engine.FusedSGD(flat, lr=0.1).grouped
    decayed = engine.FusedAdam(flat, lr=1e-3, weight_decay=0.1)          # a decay makes one group of everything
    assert decayed.grouped and [len(g["params"]) for g in decayed.param_groups] == [len(flat.params)]
    decayed.load_state_dict(sd)
    assert decayed.param_groups[0]["weight_decay"] == 0.1


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_multistep_lr_scales_every_group(kind):
    from buctd_amd import engine
    flat = engine.FlatParams(small_net())
    opt = make_fused(kind, flat, three_groups(flat.params, kind))
    lrs = [g["lr"] for g in opt.param_groups]
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[1, 2], gamma=0.1)
    opt._opt_called = True       # (no device step here: tell the scheduler that the optimizer has stepped)
    sched.step()
    assert [g["lr"] for g in opt.param_groups] == pytest.approx([0.1 * v for v in lrs])
    sched.step()
    assert [g["lr"] for g in opt.param_groups] == pytest.approx([0.01 * v for v in lrs])


def test_groups_by_name():
    from buctd_amd import engine
    net = torch.nn.Sequential()
    net.add_module("stem", torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3, bias=False), torch.nn.BatchNorm2d(8)))
    net.add_module("stage", torch.nn.Sequential(torch.nn.Conv2d(8, 8, 3), torch.nn.LayerNorm(8)))
    net.add_module("final_layer", torch.nn.Conv2d(8, 4, 1))
    names = {id(p): n for n, p in net.named_parameters()}
    rules = [("final_layer", {"lr": 1e-2}), ("stage", {"lr": 1e-3, "weight_decay": 1e-2})]
    groups = engine.groups_by_name(net, rules)
    assert [[names[id(p)] for p in g["params"]] for g in groups] == [
        ["final_layer.weight", "final_layer.bias"], ["stage.0.weight", "stage.0.bias", "stage.1.weight", "stage.1.bias"]]
    assert groups[0]["lr"] == 1e-2 and groups[1]["weight_decay"] == 1e-2           # stem.*: unmatched, left out
    # the first match wins: "" behind "final_layer" takes the rest only
    groups = engine.groups_by_name(net, [("final_layer", {"lr": 1e-2}), ("", {"lr": 1e-3})])
    assert [len(g["params"]) for g in groups] == [2, 7]
    groups = engine.groups_by_name(net, [("final_layer", {"lr": 1e-2, "weight_decay": 0.1}), ("", {"weight_decay": 0.2})],
                                   no_decay_for_norm_and_bias=True)
    got = [([names[id(p)] for p in g["params"]], g["weight_decay"], g.get("lr")) for g in groups]
    assert got == [(["final_layer.weight"], 0.1, 1e-2), (["final_layer.bias"], 0.0, 1e-2),
                   (["stem.0.weight", "stage.0.weight"], 0.2, None),
                   (["stem.1.weight", "stem.1.bias", "stage.0.bias", "stage.1.weight", "stage.1.bias"], 0.0, None)]
    flat = engine.FlatParams(net)
    opt = engine.FusedAdam(flat, groups=engine.groups_by_name(net, rules, True), decoupled_weight_decay=True)
    assert len(opt.param_groups) == 4 and all(g["decoupled_weight_decay"] for g in opt.param_groups)


def test_get_optimizer_passes_groups_through():
    from buctd_amd import engine
    from buctd_amd.config import cfg
    c = cfg.clone()
    c.defrost()
    c.TRAIN.OPTIMIZER, c.TRAIN.LR = "adam", 0.01
    net = small_net()
    opt = engine.get_optimizer(c, net, groups=[{"params": list(net[2].parameters()), "lr": 0.1}], weight_decay=0.05,
                               decoupled_weight_decay=True)
    g = opt.param_groups[0]
    assert isinstance(opt, engine.FusedAdam) and opt.grouped and len(opt.param_groups) == 1
    assert (g["lr"], g["weight_decay"], g["decoupled_weight_decay"], len(g["params"])) == (0.1, 0.05, True, 2)
    assert not engine.get_optimizer(c, small_net()).grouped
    c.TRAIN.OPTIMIZER = "sgd"
    net = small_net()
    opt = engine.get_optimizer(c, net, groups=[{"params": list(net[0].parameters())}, {"params": list(net[2].parameters()),
                                                                                      "weight_decay": 0.0}])
    assert isinstance(opt, engine.FusedSGD) and [g["weight_decay"] for g in opt.param_groups] == [c.TRAIN.WD, 0.0]
    assert opt.param_groups[0]["momentum"] == c.TRAIN.MOMENTUM


def test_get_last_layer_optimizer_freezes_all_but_the_final_layer():
    """reference lib/utils/utils.py:277-290"""
    from buctd_amd import engine
    from buctd_amd.config import cfg
    from buctd_amd.utils import utils
    net = torch.nn.Sequential()
    net.add_module("stem", torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3), torch.nn.BatchNorm2d(8)))
    net.add_module("final_layer", torch.nn.Conv2d(8, 4, 1))
    c = cfg.clone()
    c.defrost()
    c.TRAIN.LR = 0.02
    net.train()
    opt = utils.get_last_layer_optimizer(c, net)
    assert isinstance(opt, engine.FusedAdam) and opt.grouped and net.training
    assert sorted(n for n, p in net.named_parameters() if p.requires_grad) == ["final_layer.bias", "final_layer.weight"]
    assert len(opt.param_groups) == 1 and opt.param_groups[0]["lr"] == 0.02 and opt.param_groups[0]["weight_decay"] == 0
    assert [id(p) for p in opt.param_groups[0]["params"]] == [id(net.final_layer.weight), id(net.final_layer.bias)]
    assert all(opt.flat.owns(p) for p in net.parameters())
