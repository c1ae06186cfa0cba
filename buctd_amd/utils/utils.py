"""Boundary helpers of the training driver - drop-in for the pieces of reference lib/utils/utils.py the path
uses: get_optimizer (258-274), get_network_grad_flow (293-300), save_checkpoint (303-308), create_logger (220-255, without
the dataset-specific directory logic that needs the external data tree)."""
import logging
import os
import time

import torch

from ..engine import get_optimizer  # noqa: F401  (same name / signature as the reference helper)


def get_last_layer_optimizer(cfg, model):
    """reference lib/utils/utils.py:277-290, its fine-tuning entry: freeze every parameter whose name lacks 'final_layer'
    and run Adam(cfg.TRAIN.LR) over what is left - here a grouped engine.FusedAdam with that one group, so the frozen trunk
    is never read or written by a step (and its backward kernels are not launched).  The model stays as it is otherwise:
    in train mode BatchNorm running statistics keep moving, as in the reference.  `model` may be an engine.DataParallel in
    a world of one; under a gradient exchange the grouped form refuses a partly frozen arena.  A partial freeze made by
    hand (some parameters of a node frozen, others not) gives the frozen ones no .grad either: the nodes write their
    gradients to scratch (ops.grad_target), so any optimizer on the arena leaves them alone."""
    from .. import engine
    for name, param in model.named_parameters():
        if 'final_layer' not in name:
            param.requires_grad = False
    if isinstance(model, engine.DataParallel):
        flat = model.flatten()
        sync = model.sync_gradients if model._exchange else None      # a world of one exchanges nothing
    else:
        flat, sync = engine.FlatParams(model), None
    head = [p for p in flat.params if p.requires_grad]
    return engine.FusedAdam(flat, lr=cfg.TRAIN.LR, grad_sync=sync, groups=[{"params": head}])


def get_network_grad_flow(model):
    """Sum over the trainable parameters of mean |grad|, a Python float (reference lib/utils/utils.py:293-300).  When the
    model's parameters live in an engine.FlatParams arena the per-parameter means come from one launch over the gradient
    arena (engine.grad_stats) and one read-back; otherwise the reference's loop runs as it stands."""
    from .. import engine, ops
    params = [p for _, p in model.named_parameters() if p.requires_grad]
    flat = getattr(model, "flat", None)
    if not isinstance(flat, engine.FlatParams):
        flat = ops._grad_arena if isinstance(ops._grad_arena, engine.FlatParams) else None
    if flat is not None and flat.grad.is_cuda and params and all(flat.owns(p) for p in params):
        index = {id(p): i for i, p in enumerate(flat.params)}
        rows = torch.tensor([index[id(p)] for p in params], device=flat.grad.device)
        return float(engine.grad_stats(flat)["abs_mean"][rows].sum().item())
    total_avg_gradient = 0.0
    for p in params:
        total_avg_gradient += p.grad.abs().mean().item()
    return total_avg_gradient


def save_checkpoint(states, is_best, output_dir, filename='checkpoint.pth'):
    """Writes the checkpoint dict; a best-so-far run additionally leaves its bare best_state_dict as
    model_best.pth (what tools/test.py loads).  Same files as the reference helper."""
    target = os.path.join(output_dir, filename)
    torch.save(states, target)
    best = states.get('best_state_dict') if (is_best and 'state_dict' in states) else None
    if best is not None:
        torch.save(best, os.path.join(output_dir, 'model_best.pth'))
    return target


def create_logger(cfg, cfg_name, phase='train'):
    """<OUTPUT_DIR>/<dataset>/<model>/<cfg name>/ for logs and checkpoints, <LOG_DIR>/.../<cfg name>_<time>/ for
    tensorboard; returns (logger, output dir, tensorboard dir)."""
    stamp = time.strftime('%Y-%m-%d-%H-%M')
    stem = os.path.splitext(os.path.basename(cfg_name))[0]
    leaf = os.path.join(cfg.DATASET.DATASET, cfg.MODEL.NAME)
    out_dir = os.path.join(cfg.OUTPUT_DIR or 'output', leaf, stem)
    tb_dir = os.path.join(cfg.LOG_DIR or 'log', leaf, stem + '_' + stamp)
    for d in (out_dir, tb_dir):
        os.makedirs(d, exist_ok=True)
    root = logging.getLogger()
    root.setLevel(logging.INFO)
    file_handler = logging.FileHandler(os.path.join(out_dir, f'{stem}_{stamp}_{phase}.log'))
    file_handler.setFormatter(logging.Formatter('%(asctime)-15s %(message)s'))
    root.addHandler(file_handler)
    root.addHandler(logging.StreamHandler())
    return root, str(out_dir), str(tb_dir)
