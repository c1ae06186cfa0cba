"""Training runtime of the MI355X engine: flat parameter / gradient arenas, the fused Adam step and the
one-process-per-GPU data-parallel wrapper (RCCL all-reduce over xGMI).

What it replaces in the reference:
  * torch.nn.DataParallel(model).cuda() (tools/train.py:147): one process, per-iteration parameter broadcast,
    scatter / gather and reduce-add to GPU 0.  Here every rank holds resident parameters; the only per-step
    exchange is a bucketed all-reduce of the flat fp32 gradient, launched bucket by bucket on a side stream while
    the backward pass is still producing earlier layers' gradients.
  * optim.Adam(model.parameters(), lr) (lib/utils/utils.py:268-272): ~1800 tensors -> one fused kernel over the
    flat arena (buctd_adam_step), gradient averaging (1/world) folded in.
BatchNorm statistics stay per replica, like under nn.DataParallel (no SyncBN); buffers of rank 0 are the ones a
checkpoint sees (broadcast_buffers()).
"""
import contextlib
import os
import time
import weakref

import torch
import torch.distributed as dist

from . import _C
from . import nn as bnn
from . import ops

_ALIGN = 4  # floats: every tensor starts on a 16-byte boundary of the arena


class FlatParams:
    """Moves all parameters of `module` into one contiguous fp32 buffer (views keep logical shape and the
    channels_last strides of conv weights) and owns a same-layout gradient arena the backward kernels write into."""

    def __init__(self, module):
        bnn.prepare_module(module)
        self.module = module       # WeightAverage: buffers and state_dict keys of the network the arena belongs to
        self.params = []
        self.names = {id(p): n for n, p in module.named_parameters()}     # for messages (parameter groups)
        seen = set()
        for p in module.parameters():
            if id(p) not in seen:
                seen.add(id(p))
                self.params.append(p)
        if not self.params:
            raise ValueError("module has no parameters")
        dev = self.params[0].device
        self.offsets = {}
        self._aligned = {}         # id(p) -> aligned_span(p)
        off = 0
        for p in self.params:
            if p.dtype != torch.float32 or p.device != dev:
                raise ValueError("all parameters must be fp32 on one device")
            end = off + (p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN
            self.offsets[id(p)] = off
            self._aligned[id(p)] = (off, end)
            off = end
        self.numel = off
        self.flat = torch.zeros(off, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(off, dtype=torch.float32, device=dev)
        self._gviews = {}
        for p in self.params:
            v = self._view(self.flat, p)
            v.copy_(p.data)
            p.data = v
            self._gviews[id(p)] = self._view(self.grad, p)
        self.ready_cb = None
        self.optimizer = None      # weak reference to the FusedAdam / FusedSGD that steps this arena (clip_grad_norm_ asks it)
        self._clip = None          # device state of the norm clip (_GradClip), made on first use
        self._span_table = None    # int64 [P, 2] device table of the parameters' spans (grad_stats)
        ops.set_grad_arena(self)

    def _view(self, buf, p):
        o = self.offsets[id(p)]
        return torch.as_strided(buf, p.shape, p.stride(), o)

    def span(self, p):
        o = self.offsets[id(p)]
        return o, o + p.numel()

    def aligned_span(self, p):
        """p's slot of the arena: span(p) with the end rounded up to _ALIGN, i.e. with the padding behind it"""
        return self._aligned[id(p)]

    @staticmethod
    def merge_spans(spans, keys=None):
        """Ascending [start, end) spans -> (runs, the key of each run): spans that touch are merged into one run, except
        where their keys differ (the grouped optimizers: a run belongs to one group)."""
        runs, run_keys = [], []
        for (s, e), k in zip(spans, keys if keys is not None else [None] * len(spans)):
            if runs and runs[-1][1] == s and run_keys[-1] == k:
                runs[-1] = (runs[-1][0], e)
            else:
                runs.append((s, e))
                run_keys.append(k)
        return runs, run_keys

    # ops.grad_target protocol -------------------------------------------------------------
    def __call__(self, p):
        return self._gviews.get(id(p))

    def owns(self, p):
        return id(p) in self._gviews

    def grad_is_arena(self, p):
        return p.grad is not None and p.grad.data_ptr() == self._gviews[id(p)].data_ptr()

    def collect(self):
        """Make the arena hold the current gradient of every parameter (zero where there is none)."""
        for p in self.params:
            g = self._gviews[id(p)]
            if p.grad is None:
                if p.requires_grad:
                    g.zero_()
            elif not self.grad_is_arena(p):
                g.copy_(p.grad)
                p.grad = g

    def grad_runs(self):
        """Contiguous [start, end) element runs of the arena that cover exactly the parameters holding a gradient right now
        (p.grad is not None) - torch.optim skips every other parameter entirely (no weight decay, no momentum), e.g.
        TransPose's frozen sine pos_embedding (transpose_h.py:129; a learnable one has a gradient like any weight) and
        constructed-but-unused modules.  One run when every parameter has a gradient (the usual case)."""
        aligned = self._aligned
        return self.merge_spans([aligned[id(p)] for p in self.params if p.grad is not None])[0]


class _GradClip:
    """Device state of the gradient-norm clip of one arena: the fp64 sum of squares, the fp32 coefficient and norm, and the
    reduction's workspace.  measure() enqueues the reduction (buctd_grad_sumsq over the arena's gradient runs) and the
    finalize step (buctd_grad_clip_coef); nothing comes back to the host."""

    def __init__(self, flat):
        dev = flat.flat.device
        self.sumsq = torch.zeros(1, dtype=torch.float64, device=dev)
        self.coef = torch.ones(1, dtype=torch.float32, device=dev)
        self.norm = torch.zeros(1, dtype=torch.float32, device=dev)
        self.workspace = None

    def measure(self, flat, gscale, max_norm, runs=None):
        """runs: the spans to measure (the grouped optimizers: what this step updates); None = the arena's gradient runs"""
        if runs is None:
            runs = flat.grad_runs()
        if runs:
            need = ops.grad_sumsq_workspace(runs) // 8
            if self.workspace is None or self.workspace.numel() < need:
                self.workspace = torch.empty(need, dtype=torch.float64, device=self.sumsq.device)
            ops.grad_sumsq(flat.grad, runs, self.sumsq, self.workspace)
        else:
            self.sumsq.zero_()         # no parameter holds a gradient: torch's norm of nothing is 0
        ops.grad_clip_coef(self.sumsq, gscale, max_norm, self.coef, self.norm)
        return runs


def _arena_clip(flat):
    if flat._clip is None:
        flat._clip = _GradClip(flat)
    return flat._clip


class _NormClipOption:
    """max_grad_norm of FusedAdam / FusedSGD: torch.nn.utils.clip_grad_norm_(parameters, max_grad_norm) folded into step().
    None / 0 is off (the plain step kernels, nothing else runs).  With a value, step() reduces the squared gradient of the
    arena's gradient runs after collect() and grad_sync() - so under engine.DataParallel the norm is that of the averaged
    gradient, what one process over the whole batch would clip - keeps norm and coefficient on the device, and the step
    kernel multiplies the gradient by gscale * coef as it reads it.  An attribute, not optimizer state: state_dict() does
    not carry it."""

    def _init_clip(self, flat, max_grad_norm):
        self.max_grad_norm = max_grad_norm
        self._last_clip = False
        flat.optimizer = weakref.ref(self)

    def _clip_coef(self, gscale, runs=None):
        """-> the device coefficient for this step's kernels, or None when the option is off"""
        m = self.max_grad_norm
        if m is None or m == 0:
            self._last_clip = False
            return None
        if not m > 0:
            raise ValueError(f"max_grad_norm must be positive (or None / 0 for no clipping), got {m!r}")
        clip = _arena_clip(self.flat)
        clip.measure(self.flat, gscale, float(m), runs)
        self._last_clip = True
        return clip.coef

    @property
    def last_grad_norm(self):
        """norm of the (averaged) gradient before the clip, as the last clipped step() measured it: a 0-d fp32 device tensor,
        overwritten by the next clipped step (clone it to keep it); None when the last step did not clip"""
        return self.flat._clip.norm.view(()) if self._last_clip else None

    @property
    def last_clip_coef(self):
        """min(1, max_grad_norm / (norm + 1e-6)) of the last clipped step(): 0-d fp32 device tensor, or None"""
        return self.flat._clip.coef.view(()) if self._last_clip else None


class _Live:
    """What a grouped step works on while the set of parameters holding a gradient stays the same: the chunk table in device
    memory, the merged spans the norm clip measures, the groups that step and the parameters that are stepped."""

    def __init__(self, table, runs, groups, ids):
        self.table, self.runs, self.groups, self.ids = table, runs, groups, ids


class _ParamGroups:
    """The grouped form of FusedAdam / FusedSGD (groups=[...], torch's param_groups on the flat arena).

    A step updates exactly the parameters that belong to a group and hold a gradient right now - FlatParams.grad_runs()
    restricted to the group members - as ONE launch of buctd_adam_step_groups / buctd_sgd_step_groups over a chunk table
    (buctd_step_chunks) that lives in device memory.  The table is built and uploaded when the set of live parameters
    changes and cached on that set, so a steady-state step is one launch and no copy; the hyper-parameters travel in the
    kernel arguments, so a scheduler that edits param_groups[i]['lr'] needs nothing else.  Arena parameters in no group and
    the slots of parameters without a gradient in the parameter / moment / momentum arenas are never read or written; the
    padding that fills a stepped parameter's last 16 bytes is part of its span and keeps its zeros (zero gradient, zero
    moments)."""

    def _check_groups(self, flat, groups, grad_sync):
        who = type(self).__name__
        groups = [dict(g) for g in groups]
        if not groups:
            raise ValueError(f"{who}: groups is empty")
        if len(groups) > _C.STEP_MAX_GROUPS:
            raise ValueError(f"{who}: {len(groups)} parameter groups, at most {_C.STEP_MAX_GROUPS} fit one launch")
        owner = {}
        for gi, g in enumerate(groups):
            ps = g.get("params", [])
            g["params"] = ps = [ps] if isinstance(ps, torch.Tensor) else list(ps)
            for p in ps:
                if not isinstance(p, torch.Tensor) or not flat.owns(p):
                    shape = tuple(p.shape) if isinstance(p, torch.Tensor) else type(p).__name__
                    raise ValueError(f"{who}: group {gi} holds a parameter of shape {shape} that is not in the arena")
                if id(p) in owner:
                    raise ValueError(f"{who}: parameter {flat.names.get(id(p), '?')!r} is in group {owner[id(p)]} and in "
                                     f"group {gi}")
                owner[id(p)] = gi
        if grad_sync is not None:
            for p in flat.params:
                if id(p) not in owner or not p.requires_grad:
                    what = "is in no group" if id(p) not in owner else "is frozen"
                    raise ValueError(f"{who}: parameter {flat.names.get(id(p), '?')!r} {what}; with a gradient exchange "
                                     "(grad_sync) the grouped form needs every arena parameter in a group and trainable")
        return groups, owner

    def _init_groups(self, owner):
        flat = self.flat
        self._members = [(p, owner[id(p)]) for p in flat.params if id(p) in owner]     # in arena order
        self._live = None
        self._live_key = None
        self._stepped = set()          # ids of the parameters that carry optimizer state (torch: those stepped at least once)
        self.table_builds = 0          # chunk tables built and uploaded so far: one per change of the live set

    def _live_set(self):
        key = bytes(p.grad is not None for p, _ in self._members)
        if key == self._live_key:
            return self._live
        flat = self.flat
        live = [(p, gi) for p, gi in self._members if p.grad is not None]
        spans = [flat.aligned_span(p) for p, _ in live]
        runs, owners = flat.merge_spans(spans, [gi for _, gi in live])      # the chunk table: a run belongs to one group
        table = None
        if runs:
            table = ops.step_chunk_table(ops.step_chunks(runs, owners, flat.numel), flat.flat.device)
            self.table_builds += 1
        self._live = _Live(table, flat.merge_spans(spans)[0], sorted(set(owners)), {id(p) for p, _ in live})
        self._live_key = key
        return self._live


class _FusedOptimizer(_NormClipOption, _ParamGroups, torch.optim.Optimizer):
    """What FusedAdam and FusedSGD share: the arena, step() around their launches, zero_grad() and torch's checkpoint format
    in both directions.  For a checkpoint the plain form is one group that holds every arena parameter.  A subclass names
    its state arenas (_slots) and supplies the launches and the checkpoint hooks listed at the end of this class."""

    avg = None      # the engine.WeightAverage attached to this optimizer: step() ends with avg.update()
    _slots = ()     # (key of torch's per-parameter state, attribute that holds its arena - laid out like the parameters)

    def __init__(self, flat, groups, defaults, grad_sync, max_grad_norm):
        """groups: torch's param_groups for the grouped form (_ParamGroups), None for the plain one"""
        if not isinstance(flat, FlatParams):
            raise TypeError(f"{type(self).__name__} works on an engine.FlatParams arena")
        self.grouped = groups is not None
        if self.grouped:
            groups, owner = self._check_groups(flat, groups, grad_sync)
        super().__init__(groups if self.grouped else flat.params, defaults)
        self.flat = flat
        if self.grouped:
            self._init_groups(owner)
        self._init_clip(flat, max_grad_norm)       # the gradient-norm clip folded into step(): _NormClipOption
        self.grad_sync = grad_sync  # callable returning the gradient scale (1/world) after syncing
        self.step_count = 0
        self.zeroed = 0             # zero_grad() calls (StepGraph: the gradient views a capture installed are gone)

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise NotImplementedError("closures are not used on the BUCTD path")
        flat = self.flat
        flat.collect()
        gscale = self.grad_sync() if self.grad_sync is not None else 1.0
        if self.grouped:
            live = self._live_set()
            coef = self._clip_coef(gscale, live.runs)
            self.step_count += 1
            written = live.table is not None       # no group member holds a gradient: torch's optimizers do nothing either
            if written:
                self._stepped |= live.ids
                self._step_groups(live, gscale, coef)
        else:
            self._step_plain(gscale, self._clip_coef(gscale))
            written = True
        if written:
            ops.weights_updated()  # the kernel wrote the parameters through raw pointers: prepared filter images are stale
            ops.refresh_prepared(flat.flat.device)    # ... and are rebuilt here, by one launch behind the step kernel
            if flat.flat.is_cuda:
                ops.acc_pool.reset(flat.flat.device)  # BatchNorm accumulators of the step: one fill, every stream is joined here
        if self.avg is not None:
            self.avg.update()      # the averaged weights follow the step: one launch behind it (WeightAverage)

    def zero_grad(self, set_to_none=True):
        self.zeroed += 1
        for p in self.flat.params:
            p.grad = None

    def state_dict(self):
        """torch's checkpoint format: the per-parameter state keyed by the parameter's index in the concatenation of the
        param_groups, and the groups with every key that torch's optimizer reads from one."""
        fill = self._group_defaults()
        state, groups, idx = {}, [], 0
        for gi, g in enumerate(self.param_groups):
            ids = []
            for p in g["params"]:
                if self._has_state(p, gi):
                    state[idx] = self._param_state(p, gi)
                ids.append(idx)
                idx += 1
            d = {k: v for k, v in g.items() if k != "params"}
            for k, v in fill.items():
                d.setdefault(k, v)
            d["params"] = ids
            groups.append(d)
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd):
        """Takes a state_dict of the matching torch optimizer (the grouped form: with the same groups).  Everything is
        checked before anything is written; a parameter that comes without state gets zeros."""
        for _, src in zip(self.param_groups, sd["param_groups"]):
            self._refuse_group(src)
        self._load_state(sd)
        for g, src in zip(self.param_groups, sd["param_groups"]):
            g.update({k: v for k, v in src.items() if k != "params"})

    def _load_state(self, sd):
        entries = self._entries(sd)
        for _, p, st, label in entries:
            for key, _ in self._slots if st is not None else ():
                if tuple(st[key].shape) != tuple(p.shape):
                    raise ValueError(f"optimizer state of parameter {label}: shape {tuple(st[key].shape)} != {tuple(p.shape)}")
        self._load_counters(entries)
        for key, attr in self._slots:
            arena = getattr(self, attr)
            for _, p, st, _ in entries if arena is not None else ():
                view = self.flat._view(arena, p)
                if st is None:
                    view.zero_()
                else:
                    view.copy_(st[key])
        if self.grouped:
            self._stepped = {id(p) for _, p, st, _ in entries if st is not None}

    def _entries(self, sd):
        """[(group index, parameter, its state or None, the parameter's name in a message)] of a torch-format state_dict.
        The grouped form wants its own group layout; the plain form reads the state by arena index."""
        who, state = type(self).__name__, sd.get("state", {})

        def state_of(i):
            st = state.get(i, state.get(str(i)))
            return None if st is None or all(st.get(key) is None for key, _ in self._slots) else st
        if not self.grouped:
            return [(0, p, state_of(i), i) for i, p in enumerate(self.flat.params)]
        if "state" not in sd or len(sd["param_groups"]) != len(self.param_groups):
            raise ValueError(f"{who}: the state_dict has {len(sd.get('param_groups', []))} parameter groups, this optimizer "
                             f"{len(self.param_groups)}")
        out = []
        for gi, (g, src) in enumerate(zip(self.param_groups, sd["param_groups"])):
            if len(src["params"]) != len(g["params"]):
                raise ValueError(f"{who}: group {gi} of the state_dict has {len(src['params'])} parameters, this optimizer's "
                                 f"{len(g['params'])}")
            out += [(gi, p, state_of(i), repr(self.flat.names.get(id(p), "?"))) for p, i in zip(g["params"], src["params"])]
        return out

    def _has_state(self, p, gi):
        """whether a checkpoint carries state for p: torch keeps state for the parameters it has stepped"""
        return id(p) in self._stepped if self.grouped else self.step_count > 0

    def _param_state(self, p, gi):
        return {key: self.flat._view(getattr(self, attr), p).clone() for key, attr in self._slots}

    # What a subclass supplies:
    #   _step_plain(gscale, coef)         count the step and launch it over the arena
    #   _step_groups(live, gscale, coef)  count the step of the groups live.groups, launch it over the chunk table live.table
    #   _group_defaults()                 the keys a written param_group gets where it lacks them
    #   _refuse_group(src)                ValueError for a loaded param_group that asks for what the class does not implement
    #   _load_counters(entries)           refuse state the class cannot hold, then set the step counters from it


def _torch_defaults(torch_class):
    return torch_class([torch.zeros(1)], lr=1e-3).defaults      # the keys this torch's optimizer reads from a group


class FusedAdam(_FusedOptimizer):
    """torch.optim.Adam(lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0) semantics on the flat arena.

    One step counter for the whole arena, and every step updates the whole arena: a parameter without a gradient is stepped
    with a zero gradient.  While its moments are zero that leaves it bit-unchanged (frozen parameters, modules that are
    constructed but never called, the alignment padding) - the same as torch.optim.Adam, which skips it.  A parameter that
    gains or loses its gradient in the middle of a run differs from torch: torch counts the steps of each parameter on its
    own (its bias corrections start at that parameter's first gradient) and leaves a parameter alone whenever its gradient
    is None, while here the bias corrections follow the arena's counter and the moments of a parameter that lost its
    gradient keep decaying into it.

    The grouped form (groups=[{"params": [...], "lr": ..., "weight_decay": ..., "betas": ..., "eps": ...}, ...] as torch
    takes them, or a non-zero weight_decay, which makes one group of every parameter) lifts these deviations: see
    _ParamGroups.  weight_decay is torch.optim.Adam's coupled decay, with decoupled_weight_decay torch.optim.AdamW's.  Every
    group keeps its own step counter, which advances on the steps in which at least one of its parameters holds a gradient;
    a parameter without a gradient is left alone, moments included.  What remains of the deviation is inside a group:
    parameters of one group that gain or lose their gradients at different times share that group's counter (torch counts
    per parameter) - put parameters that are unfrozen at different times into different groups.  Without groups and with
    weight_decay 0 nothing of this applies: the class is the plain one above."""

    _slots = (("exp_avg", "exp_avg"), ("exp_avg_sq", "exp_avg_sq"))

    def __init__(self, flat, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, grad_sync=None, max_grad_norm=None, *, groups=None,
                 weight_decay=0.0, decoupled_weight_decay=False):
        defaults = dict(lr=lr, betas=betas, eps=eps)
        if groups is None and weight_decay != 0 and isinstance(flat, FlatParams):
            groups = [{"params": flat.params}]     # a decay makes one group of every parameter
        if groups is not None:
            defaults.update(weight_decay=weight_decay, decoupled_weight_decay=bool(decoupled_weight_decay))
        super().__init__(flat, groups, defaults, grad_sync, max_grad_norm)
        if self.grouped:
            self.group_steps = [0] * len(self.param_groups)
        self.exp_avg = torch.zeros_like(flat.flat)
        self.exp_avg_sq = torch.zeros_like(flat.flat)

    def _step_plain(self, gscale, coef):
        self.step_count += 1
        g = self.param_groups[0]
        ops.adam_step(self.flat.flat, self.flat.grad, self.exp_avg, self.exp_avg_sq, g["lr"], g["betas"][0],
                      g["betas"][1], g["eps"], self.step_count, gscale, coef)

    def _step_groups(self, live, gscale, coef):
        for gi in live.groups:
            self.group_steps[gi] += 1
        table = (_C.AdamGroup * len(self.param_groups))()
        for t, g, n in zip(table, self.param_groups, self.group_steps):
            t.lr, t.beta1, t.beta2, t.eps, t.weight_decay = g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"]
            t.decoupled, t.step = int(bool(g["decoupled_weight_decay"])), n
        ops.adam_step_groups(self.flat.flat, self.flat.grad, self.exp_avg, self.exp_avg_sq, live.table, table, gscale, coef)

    # Checkpoints: torch.optim.Adam's format (what the reference stores under checkpoint['optimizer'], tools/train.py:243-266),
    # per-parameter 'step' / 'exp_avg' / 'exp_avg_sq'; a parameter's step is its group's counter (the plain form: the arena's).
    # Loading accepts a torch.optim.Adam state_dict (reference checkpoints) or this class's round-1 flat format; the grouped
    # form a torch.optim.Adam / AdamW state_dict with the same groups.
    def _param_state(self, p, gi):
        step = self.group_steps[gi] if self.grouped else self.step_count
        return {"step": torch.tensor(float(step)), **super()._param_state(p, gi)}

    def _group_defaults(self):
        if not self.grouped:
            return {"weight_decay": 0, "amsgrad": False, "maximize": False}
        decoupled = any(g["decoupled_weight_decay"] for g in self.param_groups)
        return _torch_defaults(torch.optim.AdamW if decoupled else torch.optim.Adam)

    def _refuse_group(self, src):
        if not self.grouped and src.get("weight_decay", 0) not in (0, 0.0):
            raise ValueError("FusedAdam implements Adam without weight decay (the BUCTD recipe)")
        for k in ("amsgrad", "maximize"):
            if src.get(k):
                raise ValueError(f"FusedAdam does not implement {k}")

    def _load_state(self, sd):
        if self.grouped or "state" in sd:
            return super()._load_state(sd)
        self.step_count = int(sd["step"])          # round-1 private format: flat arenas
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])

    def _load_counters(self, entries):
        steps = [set() for _ in self.param_groups]
        for gi, _, st, _ in entries:
            if st is not None:
                steps[gi].add(int(float(st["step"])))
        for gi, ss in enumerate(steps):
            if len(ss) > 1 and not self.grouped:
                raise ValueError("FusedAdam keeps one step counter: per-parameter steps differ in this state_dict")
            if len(ss) > 1:
                raise ValueError(f"FusedAdam keeps one step counter per group: the steps of group {gi} differ in this "
                                 f"state_dict ({sorted(ss)})")
        counts = [ss.pop() if ss else 0 for ss in steps]
        if self.grouped:
            self.group_steps = counts
        self.step_count = max(counts)


class FusedSGD(_FusedOptimizer):
    """torch.optim.SGD(lr, momentum, weight_decay, nesterov) semantics on the flat arena (one kernel per step) - the 'sgd'
    branch of the reference's get_optimizer (lib/utils/utils.py:260-267).  Reads and writes torch.optim.SGD state_dicts.

    With groups=[{"params": [...], "lr": ..., "momentum": ..., "weight_decay": ..., "nesterov": ...}, ...] the grouped form
    (_ParamGroups): every group steps with its own values and a step is one launch however many gradient runs there are
    (the plain form launches once per run)."""

    _slots = (("momentum_buffer", "buf"),)

    def __init__(self, flat, lr=1e-3, momentum=0.0, weight_decay=0.0, nesterov=False, grad_sync=None, max_grad_norm=None, *,
                 groups=None):
        if nesterov and momentum <= 0:
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        if groups is not None:
            groups = [dict(g) for g in groups]
        for gi, g in enumerate(groups or ()):
            if g.get("nesterov", nesterov) and g.get("momentum", momentum) <= 0:
                raise ValueError(f"FusedSGD: group {gi}: Nesterov momentum requires a momentum and zero dampening")
            if g.get("dampening", 0) not in (0, 0.0):
                raise ValueError(f"FusedSGD: group {gi}: dampening = 0 is what FusedSGD implements")
        super().__init__(flat, groups, dict(lr=lr, momentum=momentum, dampening=0, weight_decay=weight_decay, nesterov=nesterov),
                         grad_sync, max_grad_norm)
        self.buf = torch.zeros_like(flat.flat) if any(g["momentum"] for g in self.param_groups) else None

    def _step_plain(self, gscale, coef):
        g = self.param_groups[0]
        # torch.optim.SGD touches only parameters that hold a gradient: a parameter with p.grad None keeps its value (no
        # weight decay) and its momentum buffer.  A zero momentum buffer makes "buf = momentum * buf + g" the first-step
        # initialisation "buf = g" (dampening 0), so parameters that join later need no flag of their own.
        for s, e in self.flat.grad_runs():
            ops.sgd_step(self.flat.flat[s:e], self.flat.grad[s:e], None if self.buf is None else self.buf[s:e], g["lr"],
                         g["momentum"], g["weight_decay"], g["nesterov"], False, gscale, coef)
        self.step_count += 1

    def _step_groups(self, live, gscale, coef):
        table = (_C.SgdGroup * len(self.param_groups))()
        for t, g in zip(table, self.param_groups):
            t.lr, t.momentum, t.weight_decay, t.nesterov = g["lr"], g["momentum"], g["weight_decay"], int(bool(g["nesterov"]))
        # a zero momentum buffer makes "buf = momentum * buf + g" the first-step "buf = g", as in the plain form
        ops.sgd_step_groups(self.flat.flat, self.flat.grad, self.buf, live.table, table, gscale, coef)

    def load_state_dict(self, sd):
        super().load_state_dict(sd)
        if self.buf is None and any(g["momentum"] for g in self.param_groups):
            self.buf = torch.zeros_like(self.flat.flat)    # a loaded group brought a momentum

    def _has_state(self, p, gi):
        momentum = self.param_groups[gi]["momentum"] if self.grouped else self.buf is not None
        return bool(momentum) and super()._has_state(p, gi)        # torch: no state without momentum

    def _group_defaults(self):
        return _torch_defaults(torch.optim.SGD)    # the plain form lacks maximize, foreach, differentiable, fused

    def _refuse_group(self, src):
        if src.get("dampening", 0) not in (0, 0.0):
            raise ValueError("FusedSGD implements dampening = 0 (the reference's recipe)")
        if src.get("maximize"):
            raise ValueError("FusedSGD does not implement maximize")

    def _load_counters(self, entries):
        loaded = any(st is not None for _, _, st, _ in entries)
        if loaded and self.buf is None:
            raise ValueError("FusedSGD was built without momentum but the state_dict carries momentum buffers")
        self.step_count = 1 if loaded else 0


class GradBuckets:
    """Contiguous slices of the gradient arena, cut so that a bucket closes when the backward pass (which
    produces gradients roughly in reverse registration order) has written all of its tensors."""

    def __init__(self, flat, bucket_bytes=48 << 20):
        self.flat = flat
        target = bucket_bytes // 4
        self.buckets = []  # (start, end, set(param ids))
        cur_ids, cur_end, cur_start = set(), None, None
        def close():
            nonlocal cur_ids, cur_end
            if cur_ids:
                self.buckets.append((cur_start, cur_end, cur_ids))
            cur_ids, cur_end = set(), None

        for p in reversed(flat.params):
            s, e = flat.aligned_span(p)
            if e - s >= target:
                # a tensor as large as a bucket (CoAM fc_o: 191 MB of the 462 MB) travels alone, so that its
                # all-reduce starts the moment its gradient GEMM is enqueued instead of waiting for neighbours
                close()
                self.buckets.append((s, e, {id(p)}))
                continue
            if cur_end is None:
                cur_end = e
            cur_start = s
            cur_ids.add(id(p))
            if cur_end - cur_start >= target:
                close()
        close()
        self.of_param = {}
        for i, (_, _, ids) in enumerate(self.buckets):
            for pid in ids:
                self.of_param[pid] = i


class DataParallel(torch.nn.Module):
    """Drop-in for torch.nn.DataParallel in tools/train.py:147 / tools/test.py:134 under a
    one-process-per-GPU launch (torchrun): exposes .module, forwards to it, keeps replicas identical.

    Without an initialised process group (single GPU) it is a transparent wrapper."""

    def __init__(self, module, device_ids=None, bucket_bytes=48 << 20, overlap=True, exchange_in_world_of_one=False):
        super().__init__()
        self.module = module
        self.flat = None
        self.world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        self.rank = dist.get_rank() if self.world > 1 else 0
        # exchange_in_world_of_one: run the whole gradient exchange (buckets, communication stream, collectives) in an
        # initialised process group of ONE rank too - the sum over one rank is the identity, so the step must equal the
        # plain engine's bit for bit; the hardware test of the RCCL transport on a single-GPU box
        self._exchange = self.world > 1 or (exchange_in_world_of_one and dist.is_available() and dist.is_initialized())
        self.bucket_bytes = bucket_bytes
        self.overlap = overlap
        self._handles = []
        self._pending = False
        self._dirty = False
        self._entry_stream = None
        self._comm_stream = None
        self._collective_in_stream = False
        # bench.py: set to a list to get one (bucket index, bytes, start event, end event) per bucket exchange on the
        # communication stream (timing events; None = off, the production setting)
        self.bucket_trace = None

    # -- construction-time helpers ---------------------------------------------------------
    def cuda(self, device=None):
        self.module.cuda(device)
        return self

    def flatten(self):
        if self.flat is None:
            self.flat = FlatParams(self.module)
            if self._exchange:
                dist.broadcast(self.flat.flat, src=0)
                self.broadcast_buffers()
                self.buckets = GradBuckets(self.flat, self.bucket_bytes)
                self._collective_in_stream = self.flat.flat.is_cuda and dist.get_backend() == "nccl"
                if self.overlap and self.flat.flat.is_cuda:
                    # the exchange runs at the HIGHEST stream priority: an RCCL kernel occupies a few CUs per channel and
                    # must not queue behind the four compute streams' workgroups (it would start when they drain, i.e.
                    # exposed); what it takes away from them is its channel count (RCCL's default: <= 32 CUs of 256)
                    dev = self.flat.flat.device
                    self._comm_stream = _comm_streams.get(dev.index) or torch.cuda.Stream(device=dev, priority=-1)
                    # HIP stream budget: the default runtime serves FOUR hardware queues and any fifth stream costs 25-32 %
                    # (DESIGN.md 3.12, 6).  With the communication stream the compute side gets main + ONE branch stream
                    # (the two group-launch families of a HighResolutionModule, the fuse rows) + the weight-gradient stream.
                    ops.set_branch_max(1)
                    ops.set_grad_ready_callback(self._grad_ready)
        return self.flat

    def broadcast_buffers(self):
        """rank 0's BatchNorm running statistics win, like replica 0 under nn.DataParallel."""
        if self._exchange:
            for b in self.module.buffers():
                dist.broadcast(b, src=0)

    def forward(self, *args, **kwargs):
        if self._exchange and self.flat is not None:
            self._start_step()
        return self.module(*args, **kwargs)

    # -- gradient exchange -----------------------------------------------------------------
    def _start_step(self):
        self._handles = []
        self._dirty = False
        nb = len(self.buckets.buckets)
        self._ready = [set() for _ in range(nb)]       # parameter ids whose gradient is final, per bucket
        self._streams = [dict() for _ in range(nb)]    # streams that produced gradient work of the bucket
        self._launched = [False] * nb
        self._pending = True
        if self.flat.flat.is_cuda:
            # the stream the backward pass is entered on: autograd replays nodes of the main path here
            self._entry_stream = torch.cuda.current_stream(self.flat.flat.device)

    MAX_HIP_STREAMS = 4      # main + branch + weight-gradient + communication (the hardware queues of the default runtime)

    _budget_warned = False

    def _check_stream_budget(self, device):
        """a PERFORMANCE condition, checked from autograd callbacks: it warns once, it never raises"""
        n = 1 + len(ops.compute_streams(device)) + (1 if self._comm_stream is not None else 0)
        if n > self.MAX_HIP_STREAMS and not DataParallel._budget_warned:
            DataParallel._budget_warned = True
            import warnings
            warnings.warn(f"{n} HIP streams on {device} (main + {len(ops.compute_streams(device))} compute + communication): "
                          "more than four hardware queues cost 25-32 % (DESIGN.md 6)", RuntimeWarning, stacklevel=2)

    def _launch(self, i):
        s, e, _ = self.buckets.buckets[i]
        view = self.flat.grad[s:e]
        self._launched[i] = True
        if self._comm_stream is not None:
            self._check_stream_budget(view.device)
            # one event per stream that wrote into this bucket, recorded now: stream order makes it cover the
            # bucket's kernels on that stream (and nothing of streams that did not contribute)
            streams = dict(self._streams[i])
            for st in (torch.cuda.current_stream(view.device), self._entry_stream):
                streams[st.cuda_stream] = st
            for st in streams.values():
                ev = torch.cuda.Event()
                ev.record(st)
                self._comm_stream.wait_event(ev)
            with torch.cuda.stream(self._comm_stream):
                if self.bucket_trace is not None:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(self._comm_stream)
                if self._collective_in_stream:
                    # RCCL: a collective issued with async_op=False is enqueued on the CURRENT stream - the communication
                    # stream - and returns at once.  async_op=True would run it on the process group's own internal stream
                    # behind an event: a FIFTH HIP stream, i.e. the 25 % cliff of DESIGN.md 6 (measured with a one-rank
                    # group: 470 -> 351 images/s).  sync_gradients joins the communication stream, no handles needed.
                    dist.all_reduce(view, op=dist.ReduceOp.SUM, async_op=False)
                else:
                    self._handles.append(dist.all_reduce(view, op=dist.ReduceOp.SUM, async_op=True))
                if self.bucket_trace is not None:
                    if not self._collective_in_stream:
                        self._handles[-1].wait()      # stream-side wait only: orders e1 behind the collective
                    e1.record(self._comm_stream)
                    self.bucket_trace.append((i, 4 * (e - s), e0, e1))
        else:
            if view.is_cuda:
                ops.wait_side_stream()
            if self._collective_in_stream:
                dist.all_reduce(view, op=dist.ReduceOp.SUM, async_op=False)     # in the current stream, as above
            else:
                self._handles.append(dist.all_reduce(view, op=dist.ReduceOp.SUM, async_op=True))

    def _grad_ready(self, p):
        """Called by the backward ops right after the kernels writing p.grad were enqueued (on the current stream
        and, for weight gradients, on ops' side stream)."""
        if not self._pending:
            return
        i = self.buckets.of_param.get(id(p))
        if i is None or not self.flat.grad_is_arena(p):
            return
        if self._launched[i] or id(p) in self._ready[i]:
            # a second gradient write to an already counted parameter (shared weight, or a second backward before
            # step()): the early all-reduce would miss it -> redo everything synchronously in sync_gradients
            self._dirty = True
            return
        if p.is_cuda:
            cur = torch.cuda.current_stream(p.device)
            self._streams[i][cur.cuda_stream] = cur
            for st in ops.side_streams(p.device):
                self._streams[i][st.cuda_stream] = st
        self._ready[i].add(id(p))
        if len(self._ready[i]) == len(self.buckets.buckets[i][2]):
            self._launch(i)

    def sync_gradients(self):
        """Finish the all-reduce of every bucket; returns the scale that turns the summed gradient into the
        gradient of the global-batch mean loss (what nn.DataParallel computes)."""
        if not self._exchange:
            return 1.0
        if not self._pending:
            self._start_step()
        if self._dirty:
            # buckets already summed over the ranks cannot be summed again: drain what is in flight, reset the step state
            # (so that the next step starts clean instead of failing for ever) and tell the caller
            for h in self._handles:
                h.wait()
            if self._comm_stream is not None:
                torch.cuda.current_stream().wait_stream(self._comm_stream)
            self._handles, self._pending, self._dirty = [], False, False
            raise RuntimeError("engine.DataParallel: a parameter received a second gradient after its bucket was "
                               "counted (shared weights / gradient accumulation need overlap=False); this step's "
                               "gradients are not usable")
        if self.flat.flat.is_cuda:
            ops.wait_side_stream()          # buckets launched here see every gradient kernel enqueued so far
        for i in range(len(self.buckets.buckets)):
            if not self._launched[i]:       # not closed during backward (overlap off, or a parameter without gradient)
                self._launch(i)
        for h in self._handles:
            h.wait()
        if self._comm_stream is not None:
            torch.cuda.current_stream().wait_stream(self._comm_stream)
        self._handles, self._pending = [], False
        return 1.0 / self.world

    # (checkpoints carry the reference's 'module.' prefix through nn.Module's own state_dict: the wrapped net is `self.module`)


def get_optimizer(cfg, model, max_grad_norm=None, *, groups=None, weight_decay=None, decoupled_weight_decay=False,
                  ema_decay=None):
    """reference lib/utils/utils.py:258-274: SGD(lr, MOMENTUM, WD, NESTEROV) for 'sgd', Adam(lr) for 'adam' - here the fused
    flat-arena optimizers, wired to the data-parallel gradient exchange when `model` is an engine.DataParallel.
    max_grad_norm (or, when it is None, cfg.TRAIN.CLIP_GRAD_NORM where a configuration carries that key; 0 = off) switches
    on the gradient-norm clip inside step() - the reference's loop calls clip_grad_norm(model.parameters(), args.clip)
    between backward() and step() (lib/core/train.py:138-141).
    groups (torch's param_groups, e.g. from groups_by_name), weight_decay and decoupled_weight_decay go to the optimizers'
    grouped form; without them the two branches are the reference's: SGD decays with cfg.TRAIN.WD, Adam does not decay.
    ema_decay (or, when it is None, cfg.TRAIN.EMA_DECAY; 0 = off) attaches a WeightAverage(optimizer, decay=ema_decay) - an
    exponential moving average of the weights with warm-up, updated by every step(): `optimizer.avg`."""
    if max_grad_norm is None:
        max_grad_norm = getattr(cfg.TRAIN, "CLIP_GRAD_NORM", 0.0)
    if ema_decay is None:
        ema_decay = getattr(cfg.TRAIN, "EMA_DECAY", 0.0)
    if isinstance(model, DataParallel):
        flat, sync = model.flatten(), model.sync_gradients
    else:
        flat, sync = FlatParams(model), None
    if cfg.TRAIN.OPTIMIZER == "sgd":
        if decoupled_weight_decay:
            raise ValueError("get_optimizer: decoupled_weight_decay belongs to Adam (torch.optim.AdamW)")
        opt = FusedSGD(flat, lr=cfg.TRAIN.LR, momentum=cfg.TRAIN.MOMENTUM,
                       weight_decay=cfg.TRAIN.WD if weight_decay is None else weight_decay,
                       nesterov=cfg.TRAIN.NESTEROV, grad_sync=sync, max_grad_norm=max_grad_norm, groups=groups)
    elif cfg.TRAIN.OPTIMIZER == "adam":
        opt = FusedAdam(flat, lr=cfg.TRAIN.LR, grad_sync=sync, max_grad_norm=max_grad_norm, groups=groups,
                        weight_decay=0.0 if weight_decay is None else weight_decay,
                        decoupled_weight_decay=decoupled_weight_decay)
    else:
        return None   # the reference returns None for any other name (utils.py:259, 274)
    if ema_decay:
        WeightAverage(opt, decay=ema_decay)
    return opt


_NORM_TYPES = (torch.nn.modules.batchnorm._BatchNorm, torch.nn.LayerNorm, torch.nn.GroupNorm)


def groups_by_name(model, rules, no_decay_for_norm_and_bias=False):
    """torch-style param_groups of `model` from an ordered list of (substring, options) rules: a parameter goes to the first
    rule whose substring occurs in its name ("" matches every name), a parameter that matches none is left out - the
    grouped optimizers never touch it.  options are a group's keys (lr, weight_decay, betas, ...).  With
    no_decay_for_norm_and_bias, the weights of BatchNorm / LayerNorm / GroupNorm modules and every bias move into a twin group
    behind their rule's group, with the same options but weight_decay = 0 (the usual fine-tuning recipe).  Rules that match
    nothing give no group.  Returns the list for FusedAdam / FusedSGD / get_optimizer(groups=...)."""
    model = model.module if isinstance(model, DataParallel) else model
    norm_ids = set()
    if no_decay_for_norm_and_bias:
        for mod in model.modules():
            if isinstance(mod, _NORM_TYPES):
                norm_ids.update(id(p) for p in mod.parameters(recurse=False))
    main = [[] for _ in rules]
    twin = [[] for _ in rules]
    for name, p in model.named_parameters():
        for k, (sub, _) in enumerate(rules):
            if sub in name:
                plain = no_decay_for_norm_and_bias and (id(p) in norm_ids or name.rsplit(".", 1)[-1] == "bias")
                (twin if plain else main)[k].append(p)
                break
    groups = []
    for k, (_, options) in enumerate(rules):
        if main[k]:
            groups.append(dict(options, params=main[k]))
        if twin[k]:
            groups.append(dict(options, params=twin[k], weight_decay=0.0))
    return groups


def _arena_of(target):
    if isinstance(target, FlatParams):
        return target
    flat = getattr(target, "flat", None)           # FusedAdam / FusedSGD, a flattened engine.DataParallel
    if isinstance(flat, FlatParams):
        return flat
    raise TypeError("expected an engine.FlatParams arena (or the optimizer / DataParallel that owns one)")


@torch.no_grad()
def clip_grad_norm_(flat, max_norm):
    """torch.nn.utils.clip_grad_norm_(parameters, max_norm) (norm_type 2, error_if_nonfinite False) on the arena, for loops
    that clip between backward() and step() like the reference's (lib/core/train.py:138-141), on one device: one reduction
    over the gradient runs, the coefficient formed on the device, the runs scaled in place by it.  Returns the norm before
    the clip as a 0-d fp32 device tensor; nothing is read back.  Under a gradient exchange (an optimizer with a grad_sync)
    this point of the loop is BEFORE the exchange - the local gradient, not the averaged one, would be clipped - so it
    refuses: use the optimizer's max_grad_norm, which clips behind the exchange."""
    flat = _arena_of(flat)
    opt = flat.optimizer() if flat.optimizer is not None else None
    if opt is not None and opt.grad_sync is not None:
        raise RuntimeError("engine.clip_grad_norm_: this arena's optimizer exchanges gradients in step() (grad_sync); "
                           "clipping here would act on the gradient before the exchange - set max_grad_norm on the "
                           "optimizer (FusedAdam / FusedSGD / get_optimizer(..., max_grad_norm=...)) instead")
    if not float(max_norm) > 0:
        raise ValueError(f"max_norm must be positive, got {max_norm!r}")
    flat.collect()
    clip = _arena_clip(flat)
    for s, e in clip.measure(flat, 1.0, float(max_norm)):
        ops.scale(flat.grad[s:e], clip.coef, 1.0, out=flat.grad[s:e])
    return clip.norm.view(()).clone()


@torch.no_grad()
def grad_stats(flat):
    """{'abs_mean': [P], 'norm': [P]}: mean |grad| and ||grad||_2 of every parameter of the arena, float64 device tensors in
    flat.params order, from one launch (buctd_grad_segment_stats) - what the reference's get_network_grad_flow
    (lib/utils/utils.py:293-300) reads parameter by parameter.  The arena is collect()ed first, so a trainable parameter
    without a gradient reports zeros; a frozen one reports whatever its slot holds."""
    flat = _arena_of(flat)
    flat.collect()
    if flat._span_table is None:
        flat._span_table = torch.tensor([flat.span(p) for p in flat.params], dtype=torch.int64).to(flat.grad.device)
    P = len(flat.params)
    out = torch.empty(2, P, dtype=torch.float64, device=flat.grad.device)
    ops.grad_segment_stats(flat.grad, flat._span_table, out[0], out[1])
    return {"abs_mean": out[0], "norm": out[1]}


# ---- weight averaging on the arena (csrc/weight_avg.hip) -------------------------------------------------------------------
def avg_decay(decay, t, warmup=True):
    """effective EMA decay of update t (counting from 0): with warm-up min(decay, (1 + t) / (10 + t)) - 0.1, 2/11, 3/12, ... so
    that the first updates are not dominated by the initial weights - else decay"""
    return min(decay, (1 + t) / (10 + t)) if warmup else decay


def avg_weight(mode, decay, warmup, t):
    """w of update t in avg += w * (p - avg), as a Python float (a double; the launch rounds it once to fp32): 1 - the
    effective decay for "ema", 1 / (t + 1) for "swa" (the equal average of t + 1 samples)"""
    if mode == "swa":
        return 1.0 / (t + 1)
    return 1.0 - avg_decay(decay, t, warmup)


def avg_due(step, start_step, update_every):
    """whether the step-th optimizer step (counting from 1) is averaged"""
    return step >= start_step and step % update_every == 0


class WeightAverage:
    """An averaged copy of the weights of a flat arena: an exponential moving average (mode "ema") or SWA's equal average of
    the sampled iterates (mode "swa") - what torch.optim.swa_utils.AveragedModel keeps in a deep copy of the module, here a
    shadow buffer of the arena's layout and one launch per update (buctd_ema_update: avg += w * (p - avg) over the whole
    arena; where p == avg - frozen parameters, the sine position embedding, the padding - the bits stay).

    target: a FusedAdam / FusedSGD - the average is attached (`optimizer.avg`) and every step() ends with update(); one
    average per optimizer - or a FlatParams arena, updated by hand.
    decay, warmup: "ema" - the effective decay of update t is avg_decay(decay, t, warmup); "swa" ignores them.
    start_step, update_every: the step-th call of update() (the optimizer's steps, counting from 1) is averaged when
    step >= start_step and step % update_every == 0; the others do nothing.
    buffers: "live" - nothing is kept for module buffers, the network inside applied() runs on its current BatchNorm running
    statistics; "average" - every fp32 buffer gets a shadow, updated by the same rule in one more launch
    (buctd_ema_update_tensors) and exchanged by applied().  Integer buffers (num_batches_tracked) are left alone.

    applied(): a context that exchanges arena and shadow in place (buctd_swap: no third buffer), so that the network - the
    same module, ForwardGraph and Bf16Inference wrappers included - evaluates the averaged weights, and exchanges them back on
    exit, exception or not.  Both exchanges announce themselves like an optimizer step (ops.weights_updated +
    ops.refresh_prepared): prepared filter images, folded BatchNorms and captured forward graphs follow.
    Under engine.DataParallel every rank averages the identical weights it holds: there is nothing to exchange."""

    MODES, BUFFERS = ("ema", "swa"), ("live", "average")

    def __init__(self, target, decay=0.9998, *, mode="ema", warmup=True, update_every=1, start_step=0, buffers="live"):
        if mode not in self.MODES:
            raise ValueError(f"WeightAverage: mode is one of {self.MODES}, got {mode!r}")
        if buffers not in self.BUFFERS:
            raise ValueError(f"WeightAverage: buffers is one of {self.BUFFERS}, got {buffers!r}")
        if mode == "ema" and not 0.0 <= decay < 1.0:
            raise ValueError(f"WeightAverage: decay must lie in [0, 1), got {decay!r}")
        if int(update_every) != update_every or update_every < 1:
            raise ValueError(f"WeightAverage: update_every is a positive whole number, got {update_every!r}")
        if int(start_step) != start_step or start_step < 0:
            raise ValueError(f"WeightAverage: start_step is a whole number >= 0, got {start_step!r}")
        optimizer = target if isinstance(target, (FusedAdam, FusedSGD)) else None
        if optimizer is not None and optimizer.avg is not None:
            raise RuntimeError("WeightAverage: this optimizer already has a weight average attached (optimizer.avg); "
                               "detach() it first")
        self.flat = _arena_of(target)
        self.mode, self.decay, self.warmup = mode, float(decay), bool(warmup)
        self.update_every, self.start_step, self.buffers = int(update_every), int(start_step), buffers
        self.steps = 0             # calls of update(): the optimizer's steps
        self.num_updates = 0       # of which averaged
        self.shadow = torch.empty_like(self.flat.flat)
        self.shadow.copy_(self.flat.flat)
        self._names, self._slots, self._views, self._buffer_shadow, self._table, self._table_key = [], [], [], None, None, None
        if buffers == "average":
            self._make_buffer_shadows()
        self._applied = False
        self._optimizer = None
        if optimizer is not None:
            optimizer.avg = self
            self._optimizer = weakref.ref(optimizer)

    def detach(self):
        """take the average off its optimizer: step() no longer updates it"""
        opt = self._optimizer() if self._optimizer is not None else None
        if opt is not None and opt.avg is self:
            opt.avg = None
        self._optimizer = None

    # -- buffers ---------------------------------------------------------------------------------------------------------
    def _live_buffers(self):
        """the averaged buffers as the modules hold them now (a module may have been handed a new tensor since)"""
        return [held[leaf] for held, leaf in self._slots]

    def _make_buffer_shadows(self):
        # named_buffers()' names and order, with the dict that holds each buffer: a step looks them up without walking the tree
        self._slots, views, off, seen = [], [], 0, set()
        for prefix, mod in self.flat.module.named_modules():
            for leaf, b in mod._buffers.items():
                if b is None or id(b) in seen or not b.is_floating_point():
                    continue
                seen.add(id(b))
                name = f"{prefix}.{leaf}" if prefix else leaf
                if b.dtype != torch.float32 or not b.is_contiguous() or b.device != self.flat.flat.device:
                    raise ValueError(f"WeightAverage: buffer {name!r} is not a contiguous fp32 tensor on the arena's device")
                self._names.append(name)
                self._slots.append((mod._buffers, leaf))
                views.append((off, b.numel()))
                off += (b.numel() + _ALIGN - 1) // _ALIGN * _ALIGN
        self._buffer_shadow = torch.zeros(off, dtype=torch.float32, device=self.flat.flat.device)
        self._views = [self._buffer_shadow[o:o + n] for o, n in views]
        for b, v in zip(self._live_buffers(), self._views):
            v.copy_(b.reshape(-1))

    def _buffer_views(self):
        """the shadows of the averaged buffers, flat views into one allocation, in the order of self._names"""
        return self._views

    def _buffer_table(self):
        live = self._live_buffers()
        key = tuple(b.data_ptr() for b in live)
        if key != self._table_key:             # a buffer moved (module.to(), a new tensor assigned): the table holds addresses
            self._table = ops.avg_item_table(list(zip(live, self._buffer_views())), self.flat.flat.device)
            self._table_key = key
        return self._table

    # -- the average -----------------------------------------------------------------------------------------------------
    def weight(self):
        """w of the next averaged update (a Python float)"""
        return avg_weight(self.mode, self.decay, self.warmup, self.num_updates)

    @torch.no_grad()
    def update(self):
        """Count one optimizer step and, when it is due, fold the arena into the average: one launch, plus one over the
        buffer table with buffers="average".  Returns whether the step was averaged."""
        if self._applied:
            raise RuntimeError("WeightAverage.update() inside applied(): the arena holds the averaged weights")
        self.steps += 1
        if not avg_due(self.steps, self.start_step, self.update_every):
            return False
        w = self.weight()
        ops.ema_update(self.flat.flat, self.shadow, w)
        if self._names:
            ops.ema_update_tensors(self._buffer_table(), w)
        self.num_updates += 1
        return True

    def _exchange(self):
        ops.swap(self.flat.flat, self.shadow)
        if self._names:
            for b, s in zip(self._live_buffers(), self._buffer_views()):
                ops.swap(b, s)
        # what an optimizer step does for everything keyed on the weights
        ops.weights_updated()
        ops.refresh_prepared(self.flat.flat.device)

    @contextlib.contextmanager
    def applied(self):
        if self._applied:
            raise RuntimeError("WeightAverage.applied() is not re-entrant: the averaged weights are already in the arena")
        with torch.no_grad():
            self._exchange()
        self._applied = True
        try:
            yield self
        finally:
            with torch.no_grad():
                self._exchange()
            self._applied = False

    def _average(self):
        """(arena-layout buffer, buffer shadows or live buffers) that hold the average right now"""
        if self._applied:
            return self.flat.flat, (self._live_buffers() if self._names else [])
        return self.shadow, (self._buffer_views() if self._names else [])

    @torch.no_grad()
    def model_state_dict(self):
        """The network's state_dict() - its keys, shapes and order - with the averaged weights in place of the parameters (and
        the averaged buffers with buffers="average"; every other entry is a copy of the live one): load it into a freshly
        built network, or store it as the checkpoint to evaluate."""
        arena, bufs = self._average()
        averaged = dict(zip(self._names, bufs))
        names = {id(b): n for n, b in self.flat.module.named_buffers()}
        live = self.flat.module.state_dict(keep_vars=True)
        out = type(live)()
        if hasattr(live, "_metadata"):
            out._metadata = live._metadata         # the modules' versions, which load_state_dict reads
        for key, v in live.items():
            if self.flat.owns(v):
                out[key] = torch.as_strided(arena, v.shape, v.stride(), self.flat.offsets[id(v)]).clone()
            elif names.get(id(v)) in averaged:
                out[key] = averaged[names[id(v)]].view(v.shape).clone()
            else:
                out[key] = v.detach().clone()
        return out

    def state_dict(self):
        arena, bufs = self._average()
        return {"shadow": arena.detach().clone(), "buffer_names": list(self._names),
                "buffer_shadows": [b.detach().clone() for b in bufs], "steps": self.steps, "num_updates": self.num_updates,
                "mode": self.mode, "decay": self.decay, "warmup": self.warmup, "update_every": self.update_every,
                "start_step": self.start_step, "buffers": self.buffers}

    @torch.no_grad()
    def load_state_dict(self, sd):
        if self._applied:
            raise RuntimeError("WeightAverage.load_state_dict() inside applied()")
        if sd["mode"] not in self.MODES:
            raise ValueError(f"WeightAverage: the state_dict's mode is {sd['mode']!r}")
        if sd["buffers"] != self.buffers or list(sd["buffer_names"]) != self._names:
            raise ValueError(f"WeightAverage: the state_dict was taken with buffers={sd['buffers']!r} over "
                             f"{len(sd['buffer_names'])} buffers, this average has buffers={self.buffers!r} over "
                             f"{len(self._names)}")
        if tuple(sd["shadow"].shape) != tuple(self.shadow.shape):
            raise ValueError(f"WeightAverage: the state_dict's shadow has {sd['shadow'].numel()} elements, the arena "
                             f"{self.shadow.numel()}")
        views = self._buffer_views() if self._names else []
        for name, v, src in zip(self._names, views, sd["buffer_shadows"]):
            if src.numel() != v.numel():
                raise ValueError(f"WeightAverage: buffer {name!r} has {v.numel()} elements, the state_dict's {src.numel()}")
        self.shadow.copy_(sd["shadow"])
        for v, src in zip(views, sd["buffer_shadows"]):
            v.copy_(src.reshape(-1))
        self.steps, self.num_updates = int(sd["steps"]), int(sd["num_updates"])
        self.mode, self.decay, self.warmup = sd["mode"], float(sd["decay"]), bool(sd["warmup"])
        self.update_every, self.start_step = int(sd["update_every"]), int(sd["start_step"])


# Stream-capture error mode of the two graph classes: "thread_local" - a DataLoader's pin-memory thread (hipHostMalloc) or any
# other thread of the process may call the runtime while a step is being captured; "global" would turn such a call into a
# failed capture.  The kernels autograd's device thread launches into the capturing streams are captured either way.
_CAPTURE_MODE = "thread_local"


class StepGraph:
    """The device work of one training iteration - forward, loss, backward, gradient collection - captured ONCE as a hipGraph
    and replayed per step; the optimizer step stays an eager launch behind it (its bias corrections are launch arguments).

    Why: the eager engine enqueues ~1000-1600 kernels per step through Python (autograd nodes + ctypes calls): 23-35 ms of
    host time.  HRNet-W32 at 256x192 (BASELINE config C2) has 17 ms of GPU work per batch of 32, so the eager step is bound
    by the host; a replay is one hipGraphLaunch.  The streams the engine forks (branch streams, weight-gradient stream) become
    parallel branches of the graph; nothing about the kernels or their order on a stream changes, so a replayed step is
    bit-identical to the eager one (tests/test_gpu_step_graph.py).

    Use (what core.function.train does when handed one):  `output, loss = step(input, target, target_weight)` in place of
    forward / zero_grad / backward / optimizer.step().  The first `warmup` calls with a given input signature run the eager
    engine (they are ordinary training steps: caches, workspaces, streams and LDS limits settle); the next call captures;
    every later call copies the batch into the graph's static input buffers and replays.  A batch of another shape (the last,
    ragged batch of an epoch) runs the eager engine.  `output` and `loss` are the graph's static tensors: read or copy them
    before the next call.

    Train-mode dropout (CoAM, TransPose) needs `fresh_dropout_masks=True`: the capture hands the dropout kernels device
    seeds - slots of a table they read when they run - and each replay is preceded by one uncaptured kernel that writes the
    seeds of the next eager step there (ops.fill_seed_table), so replay n draws the masks the n-th eager step would have and
    training stays bit-identical to the eager engine; ops.manual_seed and eager steps in between (warm-up, a ragged batch)
    continue the same seed sequence.  Without it such models are refused (`allow_repeated_dropout_masks`, for measurements
    only, replays one mask forever).  Not capturable, and refused loudly: a gradient exchange over a process group (the
    buckets are launched from host callbacks)."""

    def __init__(self, model, criterion, optimizer, warmup=3, streams="single", allow_repeated_dropout_masks=False,
                 autoselect=False, fresh_dropout_masks=False):
        if streams not in ("single", "engine"):
            raise ValueError("streams: 'single' (a linear graph) or 'engine' (the engine's branch / weight-gradient streams "
                             "become parallel branches of the graph)")
        if not isinstance(optimizer, (FusedAdam, FusedSGD)):
            raise TypeError("StepGraph replays into a flat gradient arena: it needs engine.FusedAdam / FusedSGD")
        if isinstance(model, DataParallel) and model._exchange:
            raise NotImplementedError("StepGraph: the bucketed gradient exchange is launched from host callbacks and is not "
                                      "captured; run the eager engine under a process group")
        self.model, self.criterion, self.optimizer = model, criterion, optimizer
        self.warmup = int(warmup)
        self.streams = streams
        if allow_repeated_dropout_masks and fresh_dropout_masks:
            raise ValueError("StepGraph: allow_repeated_dropout_masks and fresh_dropout_masks exclude each other")
        self._allow_seeds = bool(allow_repeated_dropout_masks)     # measurement only: every replay repeats one mask
        self._fresh_masks = bool(fresh_dropout_masks)
        # autoselect: the last eager settling step and the first two replays of a signature are timed (device drained around
        # them - they are ordinary training steps on the caller's batches) and the signature keeps the faster path: a linear
        # graph wins below ~batch 32 on HRNet-W32 and loses the stream concurrency of the eager engine above
        self.autoselect = bool(autoselect)
        self._eager_s = {}
        self._eager_only = set()
        self._seen = {}
        self._graphs = {}
        self._dropout = False
        self.replays = 0

    @staticmethod
    def _signature(tensors):
        return tuple((tuple(t.shape), t.dtype, t.device) for t in tensors)

    def _forward_backward(self, x, target, weight):
        outputs = self.model(x)
        heads = outputs if isinstance(outputs, list) else [outputs]
        loss = None
        for head in heads:
            term = self.criterion(head, target, weight)
            loss = term if loss is None else loss + term
        self.optimizer.zero_grad()
        loss.backward()
        return heads[-1], loss

    def _capture(self, x, target, weight):
        dev = x.device
        flat = self.optimizer.flat
        static = [t.clone() for t in (x, target, weight)]
        bns = [m for m in self.model.modules() if isinstance(m, bnn.BatchNorm2d)]
        before = [m._pending_batches for m in bns]
        drawn = ops.seeds_drawn()
        graph = torch.cuda.CUDAGraph()
        self.optimizer.zero_grad()
        ops.begin_capture(self._allow_seeds, seeds_on=dev if self._fresh_masks else None)
        forks = ops.set_stream_forks(self.streams == "engine")
        try:
            with torch.cuda.graph(graph, capture_error_mode=_CAPTURE_MODE):
                ops.acc_pool.rebase(dev)              # the pool's ordering event becomes an edge of the graph
                out, loss = self._forward_backward(*static)
                flat.collect()                        # gradients autograd accumulated outside the arena are copied per replay
                ops.acc_pool.zero_used(dev)           # a replay leaves its statistics accumulators zeroed for the next one
                used = ops.acc_pool.used(dev)
        except BaseException:
            # a failed capture must not leave the pool ordered behind a captured event, nor gradient views of a graph that
            # does not exist, nor batch or seed counts of a step that never ran: the eager engine stays usable
            ops.set_stream_forks(*forks)
            ops.end_capture()
            ops.acc_pool.rebase(dev, ops.acc_pool.used(dev))
            self.optimizer.zero_grad()
            for m, b in zip(bns, before):
                m._pending_batches = b
            ops._seed_state["counter"] = drawn
            raise
        ops.set_stream_forks(*forks)
        seeds = ops.capture_seeds()
        keep = ops.end_capture()
        ops.acc_pool.rebase(dev, used)                # eager edge: zero before the first replay, fresh (uncaptured) event
        grads = [(p, p.grad) for p in flat.params if p.grad is not None]
        counts = [(m, m._pending_batches - b) for m, b in zip(bns, before) if m._pending_batches != b]
        for m, b in zip(bns, before):
            m._pending_batches = b                    # the capture enqueued nothing: its batches are counted per replay
        if seeds is not None:
            ops._seed_state["counter"] = drawn        # likewise its dropout draws: each replay draws them (fill_seed_table)
            if seeds[1] == 0:
                seeds = None
        return {"graph": graph, "static": static, "out": out, "loss": loss, "bn_counts": counts, "keep": keep, "clocked": 0,
                "grads": grads, "zeroed": getattr(self.optimizer, "zeroed", 0), "seeds": seeds}

    def __call__(self, x, target, weight):
        key = self._signature((x, target, weight))
        g = self._graphs.get(key)
        if g is None:
            n = self._seen.get(key, 0)
            self._seen[key] = n + 1
            if n < self.warmup or not x.is_cuda or not self.model.training or key in self._eager_only:
                drawn = ops.seeds_drawn()
                clocked = self.autoselect and x.is_cuda and n == self.warmup - 1 and n > 0
                if clocked:
                    torch.cuda.synchronize(x.device)
                    t0 = time.perf_counter()
                out, loss = self._forward_backward(x, target, weight)
                self.optimizer.step()
                if clocked:
                    torch.cuda.synchronize(x.device)
                    self._eager_s[key] = time.perf_counter() - t0
                self._dropout = self._dropout or ops.seeds_drawn() != drawn
                return out, loss
            if self._dropout and not (self._allow_seeds or self._fresh_masks):
                raise NotImplementedError("StepGraph: this model draws train-mode dropout masks; the mask seed is a launch "
                                          "argument, a replay would repeat one mask - pass fresh_dropout_masks=True or run "
                                          "the eager engine")
            g = self._graphs[key] = self._capture(x, target, weight)
        for dst, src in zip(g["static"], (x, target, weight)):
            if dst.data_ptr() != src.data_ptr():
                dst.copy_(src, non_blocking=True)
        clocked = self.autoselect and key in self._eager_s and g["clocked"] < 2
        if clocked:
            torch.cuda.synchronize(x.device)
            t0 = time.perf_counter()
        if g["seeds"] is not None:
            ops.fill_seed_table(*g["seeds"])          # stream order puts it in front of every branch of the replay
        g["graph"].replay()
        for m, c in g["bn_counts"]:
            m._pending_batches += c
        self.replays += 1
        if getattr(self.optimizer, "zeroed", 0) != g["zeroed"]:
            # somebody cleared the gradients since the capture (an eager step in between, the caller's own zero_grad): the
            # replay wrote into the arena views the capture had installed - hand them to the parameters again, or the
            # optimizer would take "no gradient" for "zero"
            for p, gr in g["grads"]:
                p.grad = gr
            g["zeroed"] = getattr(self.optimizer, "zeroed", 0)
        self.optimizer.step()
        if clocked:
            torch.cuda.synchronize(x.device)
            g["clocked"] += 1
            g["replay_s"] = min(g.get("replay_s", 1e9), time.perf_counter() - t0)
            if g["clocked"] == 2 and g["replay_s"] > self._eager_s[key]:
                # the eager engine is faster for this signature: drop the graph (its outputs stay valid tensors)
                self._eager_only.add(key)
                out, loss = g["out"], g["loss"]
                del self._graphs[key]
                return out, loss
        return g["out"], g["loss"]

    def static_inputs(self, x, target, weight):
        """The static input buffers of the graph captured for this signature (None before the capture): a loader that writes
        its batches there saves the per-step copy."""
        g = self._graphs.get(self._signature((x, target, weight)))
        return None if g is None else tuple(g["static"])


class ForwardGraph(torch.nn.Module):
    """Eval-mode forward of `module` replayed from a hipGraph, one graph per input signature - the serving path: top-down pose
    inference runs the network on the few person crops of an image (tools/inference.py, lib/core/function.py:178-336 at small
    TEST.BATCH_SIZE), where the eager engine's ~400-900 launches cost more host time than the kernels take on the GPU.

    Drop-in for the module inside validate() / dataset.pipeline.IterativeRefiner: `net = engine.ForwardGraph(net)`; calls in
    train mode, with gradients enabled, or on a CPU tensor go straight to the module.  The first `warmup` calls of a signature
    run the eager engine (filter images, folded BatchNorms and workspaces settle), the next one captures a LINEAR graph (the
    runtime re-enqueues a graph with cross-queue edges node by node: DESIGN.md 3.14l), later ones copy the input into the
    graph's static buffer and replay.  Outputs are copies by default (`static_output=True` hands out the graph's own output
    tensors: valid until the next call of the same signature).  Parameters are read at replay time, so a checkpoint loaded in
    place is picked up - but anything keyed on the weights (prepared filter images, folded BatchNorms) is rebuilt by the eager
    engine, not by a replay: engine.FusedAdam steps and in-place rewrites (load_state_dict: a sample of tensor versions is
    watched) drop the graphs automatically; `reset()` does it by hand."""

    def __init__(self, module, warmup=2, static_output=False, max_graphs=8, autoselect=True):
        super().__init__()
        self.module = module
        self.warmup, self.static_output, self.max_graphs = int(warmup), bool(static_output), int(max_graphs)
        # autoselect: right after a capture the eager forward and the replay are timed (three runs each, device drained) and
        # the signature keeps the faster one - a linear graph loses the stream concurrency of the eager engine, which is worth
        # ~10 % from 16 persons per call on (profiles/r06_forward_graph_by_batch.txt)
        self.autoselect = bool(autoselect)
        self._seen, self._graphs = {}, {}
        self._epoch = None
        self._probe = None
        self._capture_streams = []
        self.replays = 0

    def reset(self):
        self._seen, self._graphs = {}, {}

    def forward(self, x, *args, **kwargs):
        if (self.module.training or torch.is_grad_enabled() or args or kwargs or not torch.is_tensor(x) or not x.is_cuda):
            return self.module(x, *args, **kwargs)
        # an optimizer step (epoch) or an in-place rewrite of the parameters (tensor versions of a sample of them: a
        # load_state_dict bumps every one) makes the eager engine rebuild prepared filter images and folded BatchNorms - a
        # replay would not: drop the graphs
        if self._probe is None:
            ps = list(self.module.parameters()) + list(self.module.buffers())
            self._probe = ps[::max(1, len(ps) // 16)]
        epoch = self._watch()
        if epoch != self._epoch:
            self.reset()
            self._epoch = epoch
        key = (tuple(x.shape), x.dtype, x.device, x.stride())
        g = self._graphs.get(key)
        if g is None:
            n = self._seen.get(key, 0)
            self._seen[key] = n + 1
            if n < self.warmup or len(self._graphs) >= self.max_graphs:
                return self.module(x)
            g = self._graphs[key] = self._capture(x)
        if not g["use"]:
            return self.module(x)
        if g["x"].data_ptr() != x.data_ptr():
            g["x"].copy_(x, non_blocking=True)
        g["graph"].replay()
        self.replays += 1
        out = g["out"]
        if self.static_output:
            return out
        return [o.clone() for o in out] if isinstance(out, list) else out.clone()

    def _watch(self):
        """What the graphs depend on besides the input: the optimizer epoch, a sample of tensor versions, and the wrapped
        module's own `weights_stamp()` where it has one (Bf16Inference: every tensor, every BatchNorm batch count)."""
        stamp = getattr(self.module, "weights_stamp", None)
        return (ops.weights_epoch(), tuple(p._version for p in self._probe), stamp() if callable(stamp) else None)

    # ---- two lanes: independent requests beside each other -------------------------------------------------------------
    def submit(self, x):
        """Asynchronous forward for a serving loop: returns a handle at once, `handle.result()` makes the current stream wait
        and returns the output (a copy).  Requests of a captured signature alternate between `LANES` graphs that replay on
        the engine's two branch streams (no new HIP stream): the launch-bound kernels of independent requests run beside
        each other - one person per call keeps ~180 kernels of a few microseconds each in flight, far from filling the
        chip.  Submit a few requests before collecting the first.  Anything that cannot be replayed (train mode, gradients,
        a signature still settling, autoselect preferring the eager engine) is computed on the spot."""
        if (self.module.training or torch.is_grad_enabled() or not torch.is_tensor(x) or not x.is_cuda):
            return _Ready(self.module(x))
        key = (tuple(x.shape), x.dtype, x.device, x.stride())
        g = self._graphs.get(key)
        if g is None or not g["use"]:
            return _Ready(self.forward(x))          # settles / captures lane 0 (and watches the weights)
        if self._watch() != self._epoch:
            return _Ready(self.forward(x))
        lanes = g.setdefault("lanes", [g])
        while len(lanes) < self.LANES:              # further lanes: their own graph, buffers and workspaces
            lanes.append(self._capture(x, lane=len(lanes), clock=False))
        k = g["next"] = (g.get("next", -1) + 1) % self.LANES
        lane = lanes[k]
        cur = torch.cuda.current_stream(x.device)
        st = ops.lane_stream(x.device, k)
        st.wait_stream(cur)                         # x is ready; the lane's previous request has been copied out (stream order)
        with torch.cuda.stream(st):
            lane["x"].copy_(x, non_blocking=True)
            lane["graph"].replay()
            out = lane["out"]
            out = [o.clone() for o in out] if isinstance(out, list) else out.clone()
            ev = torch.cuda.Event()
            ev.record(st)
        x.record_stream(st)
        self.replays += 1
        return _Pending(out, ev, x.device)

    LANES = 2

    def _capture(self, x, lane=0, clock=True):
        static = x.clone()
        graph = torch.cuda.CUDAGraph()
        # every lane is captured on a stream of its own: the engine's scratch buffers are kept per stream, so two lanes that
        # replay beside each other never share one (the capture streams themselves never execute anything)
        if lane >= len(self._capture_streams):
            self._capture_streams.extend(torch.cuda.Stream(device=x.device) for _ in range(lane + 1 - len(self._capture_streams)))
        ops.begin_capture(allow_seeds=True)     # eval mode: the attention cores draw a seed but drop nothing (p = 0)
        forks = ops.set_stream_forks(False)
        try:
            with torch.cuda.graph(graph, stream=self._capture_streams[lane], capture_error_mode=_CAPTURE_MODE):
                out = self.module(static)
        finally:
            ops.set_stream_forks(*forks)
            keep = ops.end_capture()
        if not clock:
            return {"graph": graph, "x": static, "out": out, "keep": keep, "use": True}
        use = True
        if self.autoselect:
            import time

            def clock(fn):
                fn()
                torch.cuda.synchronize(x.device)
                t0 = time.perf_counter()
                for _ in range(3):
                    fn()
                torch.cuda.synchronize(x.device)
                return time.perf_counter() - t0
            use = clock(graph.replay) <= clock(lambda: self.module(static))
        return {"graph": graph, "x": static, "out": out, "keep": keep, "use": use}


class Bf16Inference(torch.nn.Module):
    """bf16 inference mode of a models.pose_hrnet network (with or without the preNet): eval forwards run on folded bf16
    filter images and bf16 NHWC activations, one bf16 MFMA per product with fp32 accumulation (ops_bf16,
    csrc/conv_bf16.hip; accuracy bound in DESIGN.md 8).  Opt-in: nothing else dispatches to it.

    `forward(x)` takes what the network takes (fp32 N x (3+Cc) x H x W NCHW, CPU or device) and returns fp32 heat-maps of
    the network's shape.  Calls in train mode, with gradients enabled or with extra arguments go to the network unchanged.
    Works as the `model` of core.function.validate(), inside dataset.pipeline.IterativeRefiner and under
    ForwardGraph(Bf16Inference(net)).  The folded images are built on the first eval forward and rebuilt, in place, when
    any parameter or buffer of the network changed: a tensor version or storage, the optimizer epoch
    (ops.weights_epoch(): FusedAdam / FusedSGD), or a BatchNorm's pending batch count (train-mode forwards update running
    statistics through raw pointers without a version bump).  The images live as long as the wrapper does, so graphs
    captured through it keep reading valid memory.  CoAM, TransPose and PoseResNet networks raise NotImplementedError."""

    def __init__(self, model):
        super().__init__()
        from . import ops_bf16
        self.module = model
        self._net = ops_bf16.Bf16Net(model)      # refuses unsupported networks
        # conv weights channels_last now, as the fp32 engine makes them at first use (values unchanged): otherwise the
        # preNet's first fp32 forward moves its weights, and the stamp below would repack everything once more
        bnn.prepare_module(model)
        self._tensors = list(model.parameters()) + list(model.buffers())
        self._bns = [m for m in model.modules() if isinstance(m, bnn.BatchNorm2d)]
        self._stamp = None
        self.training = model.training          # ForwardGraph and validate() look at the wrapper's own flag

    def weights_stamp(self):
        return (ops.weights_epoch(), tuple(t._version for t in self._tensors), tuple(t.data_ptr() for t in self._tensors),
                tuple(b._pending_batches for b in self._bns))

    def forward(self, x, *args, **kwargs):
        if self.module.training or torch.is_grad_enabled() or args or kwargs:
            return self.module(x, *args, **kwargs)
        stamp = self.weights_stamp()
        if stamp != self._stamp:
            self._net.repack()
            self._stamp = stamp
        return self._net.forward(x)


class _Ready:
    """A result that is already enqueued on the current stream (ForwardGraph.submit when nothing was replayed)."""

    def __init__(self, out):
        self._out = out

    def result(self):
        return self._out


class _Pending:
    """A request replaying on a lane stream: result() orders the current stream behind it."""

    def __init__(self, out, event, device):
        self._out, self._event, self._device = out, event, device

    def result(self):
        cur = torch.cuda.current_stream(self._device)
        cur.wait_event(self._event)
        for o in (self._out if isinstance(self._out, list) else [self._out]):
            o.record_stream(cur)
        return self._out


_comm_streams = {}      # device index -> the communication stream reserved by reserve_streams


def reserve_streams(device, data_parallel):
    """Create AND use the HIP streams of the engine on `device` before anything else creates streams there - in particular
    before the RCCL communicator, which opens internal streams of its own.  The runtime binds a stream to one of its four
    hardware queues when the stream is first used; the first four get a queue each, later ones share - and two busy streams
    on one queue serialise (a wait of one blocks the kernels of the other).  Measured on one MI355X with a one-rank RCCL
    group: process group first, engine streams later = 352-357 images/s; engine streams first = 479 (the plain engine: 470-479).
    data_parallel: reserve main + ONE branch stream + weight-gradient stream + communication stream (and cap the branch
    streams at one); otherwise main + the branch streams + the weight-gradient stream."""
    if device.type != "cuda":
        return
    streams = []
    if data_parallel:
        ops.set_branch_max(1)
        if device.index not in _comm_streams:
            _comm_streams[device.index] = torch.cuda.Stream(device=device, priority=-1)
    streams += ops.reserve_compute_streams(device)
    if data_parallel:
        streams.append(_comm_streams[device.index])
    probe = torch.zeros(64, device=device)
    main = torch.cuda.current_stream(device)
    for st in streams:
        st.wait_stream(main)
        with torch.cuda.stream(st):
            probe.add_(1.0)
        main.wait_stream(st)
    torch.cuda.synchronize(device)


def init_distributed():
    """One process per GPU (torchrun env: RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*). Returns (rank, world, device).
    Two TEST hooks are read here and nowhere else in the engine (tests/test_gpu_ddp.py runs several ranks on the one GPU of a
    test box): BUCTD_SINGLE_DEVICE=1 puts every rank on GPU 0, BUCTD_DIST_BACKEND picks the process-group backend ("gloo" for
    that case; the default "nccl" is RCCL on ROCm).  bench.py reads BUCTD_BENCH_* (its CPU-baseline child, first-touch priming)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if torch.cuda.is_available():
        if os.environ.get("BUCTD_SINGLE_DEVICE") == "1":   # test hook: every rank on GPU 0 (needs a non-RCCL backend)
            local = 0
        torch.cuda.set_device(local)
        device = torch.device("cuda", local)
        backend = os.environ.get("BUCTD_DIST_BACKEND", "nccl")  # "nccl" is RCCL on ROCm
    else:
        device = torch.device("cpu")
        backend = "gloo"
    if world > 1 and not dist.is_initialized():
        reserve_streams(device, data_parallel=True)     # before RCCL opens its own streams
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        dist.init_process_group(backend=backend, rank=rank, world_size=world)
    # every replica draws its own dropout masks (like the replicas of nn.DataParallel), derived from the user's seed
    ops.manual_seed(ops.mix_seed(torch.initial_seed(), rank))
    return rank, world, device
