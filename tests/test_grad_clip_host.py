"""Gradient-norm clipping, host side (no GPU): the C ABI of csrc/grad_norm.hip and of the _dscale optimizer steps, the
max_grad_norm option of engine.get_optimizer / FusedAdam / FusedSGD (an attribute, not optimizer state), and the fp64
restatement of norm and coefficient the GPU tests measure against (tests/helpers/grad_clip_ref.py) checked against
torch.nn.utils.clip_grad_norm_ itself."""
import copy
import os
import re

import numpy as np
import pytest
import torch

from tests.helpers import grad_clip_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("buctd_grad_sumsq_workspace", "buctd_grad_sumsq", "buctd_grad_clip_coef", "buctd_grad_segment_stats",
       "buctd_adam_step_dscale", "buctd_sgd_step_dscale")


def test_new_entry_points_are_declared_bound_and_exported():
    import ctypes as C
    from buctd_amd import _C
    header = open(os.path.join(ROOT, "include", "buctd_hip.h")).read()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/buctd_hip.h"
        assert name in _C.SIGNATURES, f"{name} is not bound in _C.py"
        assert hasattr(_C.lib(), name)
    # the _dscale steps are the plain steps with one more pointer in front of the stream
    for plain in ("buctd_adam_step", "buctd_sgd_step"):
        res, args = _C.SIGNATURES[plain]
        assert _C.SIGNATURES[plain + "_dscale"] == (res, args[:-1] + [C.c_void_p] + args[-1:])
    chunk = int(re.search(r"#define\s+BUCTD_GRAD_SUMSQ_CHUNK\s+(\d+)", header).group(1))
    assert chunk == _C.GRAD_SUMSQ_CHUNK == R.CHUNK and chunk % 1024 == 0


def test_workspace_is_eight_bytes_per_chunk_of_every_run():
    from buctd_amd import ops
    c = R.CHUNK
    assert ops.grad_sumsq_workspace([(0, 1)]) == 8
    assert ops.grad_sumsq_workspace([(5, 5 + c)]) == 8 and ops.grad_sumsq_workspace([(5, 6 + c)]) == 16
    assert ops.grad_sumsq_workspace([(0, c - 1), (c, 3 * c + 1), (4 * c, 4 * c + 1)]) == 8 * (1 + 3 + 1)
    assert ops.grad_sumsq_workspace([(4, 4)]) == 0 and ops.grad_sumsq_workspace([(-4, 4)]) == 0      # bad run lists
    assert ops.grad_sumsq_workspace([]) == 0


def _net():
    torch.manual_seed(11)
    return torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3), torch.nn.BatchNorm2d(8), torch.nn.Flatten(), torch.nn.Linear(8, 5))


def _cfg(optimizer, clip=None):
    from buctd_amd.config import cfg as base
    c = base.clone()
    c.defrost()
    c.TRAIN.OPTIMIZER = optimizer
    if clip is not None:
        c.TRAIN.CLIP_GRAD_NORM = clip
    c.freeze()
    return c


@pytest.mark.parametrize("name,cls", [("adam", "FusedAdam"), ("sgd", "FusedSGD")])
def test_get_optimizer_passes_the_option_through(name, cls):
    from buctd_amd import engine
    from buctd_amd.config import cfg as base
    assert "CLIP_GRAD_NORM" not in base.TRAIN, "the default tree stays the reference's: the key is read with getattr"
    opt = engine.get_optimizer(_cfg(name), _net())
    assert type(opt).__name__ == cls and not opt.max_grad_norm, "no key, no keyword: clipping is off"
    assert opt.last_grad_norm is None and opt.last_clip_coef is None
    assert engine.get_optimizer(_cfg(name), _net(), max_grad_norm=2.5).max_grad_norm == 2.5
    assert engine.get_optimizer(_cfg(name, clip=0.75), _net()).max_grad_norm == 0.75
    assert engine.get_optimizer(_cfg(name, clip=0.75), _net(), max_grad_norm=4.0).max_grad_norm == 4.0, "the keyword wins"
    assert not engine.get_optimizer(_cfg(name, clip=0.0), _net()).max_grad_norm
    wrapped = engine.DataParallel(_net())
    opt = engine.get_optimizer(_cfg(name), wrapped, max_grad_norm=1.5)
    assert opt.max_grad_norm == 1.5 and opt.grad_sync is not None and opt.flat.optimizer() is opt
    opt.max_grad_norm = None            # settable as an attribute
    assert opt.max_grad_norm is None


def test_state_dict_does_not_carry_the_option():
    from buctd_amd import engine
    for make, torch_cls, kw in ((engine.FusedAdam, torch.optim.Adam, dict(lr=1e-3)),
                                (engine.FusedSGD, torch.optim.SGD, dict(lr=0.05, momentum=0.9, weight_decay=1e-4))):
        plain = make(engine.FlatParams(_net()), **kw)
        clipped = make(engine.FlatParams(_net()), max_grad_norm=0.5, **kw)
        a, b = plain.state_dict(), clipped.state_dict()
        assert a["param_groups"] == b["param_groups"] and a["state"] == b["state"] == {}
        assert not any("norm" in k or "clip" in k for g in b["param_groups"] for k in g)
        net = _net()
        ref = torch_cls(net.parameters(), **kw)
        ref.load_state_dict(b)                          # torch reads what the clipped optimizer writes ...
        clipped.load_state_dict(ref.state_dict())       # ... and the option survives loading torch's
        assert clipped.max_grad_norm == 0.5
        with pytest.raises(TypeError):
            make(_net(), max_grad_norm=0.5, **kw)


def test_clip_grad_norm_refuses_an_arena_whose_optimizer_exchanges_gradients():
    from buctd_amd import engine
    flat = engine.FlatParams(_net())
    opt = engine.FusedSGD(flat, lr=0.1, grad_sync=lambda: 0.5)
    for target in (flat, opt):
        with pytest.raises(RuntimeError, match="max_grad_norm"):
            engine.clip_grad_norm_(target, 1.0)
    with pytest.raises(TypeError):
        engine.clip_grad_norm_(_net(), 1.0)


def test_grad_flow_of_a_model_outside_an_arena_is_the_reference_loop():
    from buctd_amd.utils.utils import get_network_grad_flow
    net = _net()
    net[3].bias.requires_grad_(False)
    want = 0.0
    for _, p in net.named_parameters():
        if p.requires_grad:
            p.grad = torch.randn_like(p)
            want += p.grad.abs().mean().item()
    assert get_network_grad_flow(net) == want


@pytest.mark.parametrize("where", ["below", "just_below", "at", "above"])
def test_fp64_statement_reproduces_torch_clip_grad_norm(where):
    gen = torch.Generator().manual_seed(5)
    shapes = [(8, 3, 3, 3), (8,), (1,), (5, 13)]
    grads = [torch.randn(s, generator=gen).float() for s in shapes]
    norm = np.sqrt(R.sumsq([g.numpy() for g in grads]))
    max_norm = {"below": 2.0 * norm, "just_below": norm + 2e-6, "at": norm, "above": 0.25 * norm}[where]
    total, coef = R.norm_coef(R.sumsq([g.numpy() for g in grads]), max_norm)
    params = [torch.nn.Parameter(torch.zeros(s, dtype=torch.float64)) for s in shapes]
    for p, g in zip(params, grads):
        p.grad = g.double()
    got = torch.nn.utils.clip_grad_norm_(params, max_norm)
    assert abs(got.item() - total) <= 1e-14 * total
    assert (coef == 1.0) == (where in ("below", "just_below")) and 0.0 < coef <= 1.0
    for p, g in zip(params, grads):
        want = g.double() * coef
        assert bool(((p.grad - want).abs() <= 1e-14 * want.abs()).all())
    # the same with a gradient scale: the norm of the scaled gradient
    total_h, coef_h = R.norm_coef(R.sumsq([g.numpy() for g in grads]), max_norm, gscale=0.5)
    for p, g in zip(params, grads):
        p.grad = g.double() * 0.5
    assert abs(torch.nn.utils.clip_grad_norm_(params, max_norm).item() - total_h) <= 1e-14 * total
    assert total_h == 0.5 * total and coef_h >= coef
    # non-finite norms go through the same expressions
    assert R.norm_coef(float("inf"), 1.0) == (float("inf"), 0.0)
    assert all(np.isnan(x) for x in R.norm_coef(float("nan"), 1.0))


def test_fp32_step_formulas_follow_torch_in_float64():
    """the fp32 restatements the GPU bars are measured with agree with torch.optim in float64 to fp32 rounding"""
    gen = torch.Generator().manual_seed(9)
    p0, g = torch.randn(257, generator=gen) * 0.01, torch.randn(257, generator=gen)
    lr, b1, b2, eps = R.ADAM_HYPER
    q = torch.nn.Parameter(p0.double())
    opt = torch.optim.Adam([q], lr=lr, betas=(b1, b2), eps=eps)
    p, m, v = p0, torch.zeros(257), torch.zeros(257)
    for step in (1, 2):
        q.grad = g.double() * 0.375
        opt.step()
        p, m, v = R.adam32(p, g, m, v, step, 0.375)
        assert ((p.double() - q.detach()).abs() / (p0.double().abs() + step * lr)).max().item() <= 4 * R.FLOOR
    lr, mu, wd = R.SGD_HYPER
    for nesterov in (False, True):
        q = torch.nn.Parameter(p0.double())
        opt = torch.optim.SGD([q], lr=lr, momentum=mu, weight_decay=wd, nesterov=nesterov)
        p, buf = p0, torch.zeros(257)
        for step in (1, 2):
            q.grad = g.double() * 0.375
            opt.step()
            p, buf = R.sgd32(p, g, buf, nesterov, 0.375)
        assert ((p.double() - q.detach()).abs() / q.detach().abs().max()).max().item() <= 4 * R.FLOOR
