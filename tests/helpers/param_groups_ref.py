"""References and cases of the grouped optimizer steps (csrc/optim_groups.hip, engine.FusedAdam / FusedSGD with groups=).

Three references, none of them the grouped kernels:
  * torch.optim.Adam / AdamW / SGD in float64 on the CPU (torch_adam64, make_torch): what the steps mean;
  * the same formulas in fp32 on the CPU in the kernels' order (adam_formula32, sgd_formula32, Formula32): their
    error against fp64 sets the measured bar, max(4 x that, 2^-23), on the scales of test_gpu_heatmap_kernels.py - p relative
    to |p| before + the updates so far, m / v / buf relative to their largest element;
  * the plain entry points (buctd_adam_step, buctd_sgd_step and their _dscale forms) on the same slices, for bit identity -
    called by the tests themselves.
"""
import math

import torch

from tests.helpers.heatmap_cases import f32
from tests.helpers.stream_cases import FLOOR, case_gen  # noqa: F401  (FLOOR: re-exported for the tests)

CHUNK = 16384                  # BUCTD_STEP_CHUNK, restated
MAX_GROUPS = 16                # BUCTD_STEP_MAX_GROUPS, restated
SPAN_LENGTHS = (4, CHUNK - 4, CHUNK, CHUNK + 4, 3 * CHUNK + 8)
GAPS = (4, 8)


def expected_chunks(runs, owners):
    """the chunk table of ascending runs as the header defines it: whole chunks from the run's first element, then the rest"""
    out = []
    for (s, e), g in zip(runs, owners):
        at = s
        while at < e:
            n = min(CHUNK, e - at)
            out.append((at, n, g))
            at += n
    return out


def layout(lengths, lead=8):
    """spans of these lengths behind `lead` elements, separated by gaps of 4 and 8 elements in turn -> ([(s, e)], total)"""
    spans, at = [], lead
    for k, n in enumerate(lengths):
        spans.append((at, at + n))
        at += n + GAPS[k % 2]
    return spans, at


def adam_hyper(k):
    """distinct (lr, beta1, beta2, eps, step) per group index"""
    return (1e-3 * (k + 1), 0.9 - 0.02 * k, 0.999 - 0.003 * k, 1e-8 * (1 + k), 1 + 3 * k)


def sgd_hyper(k):
    """(lr, momentum, nesterov, weight_decay) per group index: with and without momentum, Nesterov, decay"""
    mu = (0.9, 0.0, 0.8, 0.5)[k % 4]
    return (0.05 / (k + 1), mu, int(mu != 0.0 and k % 3 == 2), (0.0, 1e-4, 1e-2)[k % 3])


def poison(n):
    """what lies outside the spans: NaN and 1e30 in turn"""
    t = torch.full((n,), float("nan"))
    t[torch.arange(n) % 2 == 1] = 1e30
    return t


# ---- Adam with decay ----------------------------------------------------------------------------------------------------------
def adam_formula32(p, g, m, v, hyper, wd, decoupled, step, gscale):
    """the grouped Adam kernel's formula in fp32 on the CPU, in its order -> p, m, v"""
    S = lambda x: torch.tensor(f32(x), dtype=torch.float32)      # noqa: E731
    lr, b1, b2, eps = hyper
    bc1 = S(1.0 - f32(b1) ** step)
    bc2s = S(math.sqrt(1.0 - f32(b2) ** step))
    gg = g * S(gscale)
    if decoupled:
        p = p * S(1.0 - f32(lr) * f32(wd))
    elif wd != 0.0:
        gg = gg + S(wd) * p
    m = S(b1) * m + (S(1.0) - S(b1)) * gg
    v = S(b2) * v + (S(1.0) - S(b2)) * gg * gg
    denom = torch.sqrt(v) / bc2s + S(eps)
    return p - (S(lr) / bc1) * (m / denom), m, v


def torch_adam64(p, g, m, v, hyper, wd, decoupled, step, gscale):
    """torch.optim.Adam / AdamW in float64 with the fp32-rounded hyper-parameters the kernel receives -> p, m, v"""
    lr, b1, b2, eps = (f32(x) for x in hyper)
    P = torch.nn.Parameter(p.double().clone())
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([P], lr=lr, betas=(b1, b2), eps=eps, weight_decay=f32(wd), foreach=False)
    opt.state[P] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.double().clone(), "exp_avg_sq": v.double().clone()}
    P.grad = g.double() * f32(gscale)
    opt.step()
    return P.data, opt.state[P]["exp_avg"], opt.state[P]["exp_avg_sq"]


def sgd_formula32(p, g, buf, lr, mu, nesterov, wd, gscale):
    """torch.optim.SGD (dampening 0, a zero buffer stands for the first step) in fp32 on the CPU, in the kernels' order"""
    S = lambda x: torch.tensor(f32(x), dtype=torch.float32)      # noqa: E731
    gg = g * S(gscale) + S(wd) * p
    b = None
    if mu != 0.0:
        b = S(mu) * buf + gg
        gg = gg + S(mu) * b if nesterov else b
    return p - S(lr) * gg, b


# ---- engine: whole optimizers on a parameter list -------------------------------------------------------------------------
def make_torch(kind, params, groups):
    """torch.optim.Adam / AdamW / SGD over `groups` ({'params': [indices], options}) of the float64 twins `params`"""
    gs = [dict({k: v for k, v in g.items() if k != "params"}, params=[params[i] for i in g["params"]]) for g in groups]
    if kind == "sgd":
        return torch.optim.SGD(gs, lr=0.1, foreach=False)
    return (torch.optim.AdamW if kind == "adamw" else torch.optim.Adam)(gs, lr=1e-3, weight_decay=0.0, foreach=False)


class Formula32:
    """The grouped optimizers' semantics in fp32 on the CPU: per-group counters, a parameter without a gradient is skipped.
    groups: [{'params': [indices], 'lr': ..., ...}] with every option spelled out."""

    def __init__(self, kind, params, groups):
        self.kind, self.groups = kind, groups
        self.p = [p.clone().float() for p in params]
        self.a = [torch.zeros_like(p) for p in self.p]      # exp_avg / momentum buffer
        self.b = [torch.zeros_like(p) for p in self.p]      # exp_avg_sq
        self.steps = [0] * len(groups)

    def step(self, grads):
        for gi, g in enumerate(self.groups):
            live = [i for i in g["params"] if grads[i] is not None]
            if not live:
                continue
            self.steps[gi] += 1
            for i in live:
                if self.kind == "sgd":
                    self.p[i], buf = sgd_formula32(self.p[i], grads[i].float(), self.a[i], g["lr"], g["momentum"], g["nesterov"],
                                                   g["weight_decay"], 1.0)
                    if buf is not None:
                        self.a[i] = buf
                else:
                    hyper = (g["lr"], g["betas"][0], g["betas"][1], g["eps"])
                    self.p[i], self.a[i], self.b[i] = adam_formula32(self.p[i], grads[i].float(), self.a[i], self.b[i], hyper,
                                                                     g["weight_decay"], self.kind == "adamw", self.steps[gi], 1.0)


def bar(e32):
    return max(4 * e32, FLOOR)
