"""engine.StepGraph(..., fresh_dropout_masks=True): models with train-mode dropout (CoAM, TransPose) replayed from a
hipGraph.  The dropout kernels of the graph read their seeds from a device table that is refilled in front of every replay,
so replay n draws the masks of the n-th eager step: losses, outputs, parameters, BatchNorm statistics, optimizer state and
the host seed counter equal the eager engine's bit for bit, with eager steps (warm-up, a ragged batch) mixed in."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 0x5EED


def _coam_cfg(lr=1e-3):
    from buctd_amd.config import cfg as base, hrnet_extra
    c = base.clone()
    c.defrost()
    c.MODEL.NAME = "pose_hrnet_coam"
    c.MODEL.NUM_JOINTS = 14
    c.MODEL.IMAGE_SIZE = [64, 96]
    c.MODEL.HEATMAP_SIZE = [16, 24]
    c.MODEL.ATT_MODULES = [False, True, False, False]
    c.MODEL.CONDITIONAL_TOPDOWN = True
    c.MODEL.EXTRA = hrnet_extra(16, use_attention=True, modules=(1, 2, 2))
    c.DATASET.COLORED = True
    c.TRAIN.LR = lr
    c.freeze()
    return c


def _transpose_cfg():
    from oracle import cfg as ocfg
    c = ocfg.hrnet_cfg(16, 17, (64, 96), "transpose_h", use_attention=True, stage_modules=(1, 2, 2))
    c.MODEL.DIM_MODEL = 32
    c.MODEL.DIM_FEEDFORWARD = 64
    c.MODEL.ENCODER_LAYERS = 2
    return c


def _net(kind, cfg, device):
    from buctd_amd import models
    mod = models.pose_hrnet_coam if kind == "coam" else models.transpose_h
    torch.manual_seed(11)
    return mod.get_pose_net(cfg, is_train=True).to(device)


def _engines(kind, cfg, device, n=2):
    from buctd_amd import engine
    from buctd_amd.core.loss import JointsMSELoss
    net = _net(kind, cfg, device)
    out = []
    for i in range(n):
        model = engine.DataParallel(net if i == 0 else copy.deepcopy(net))
        opt = engine.get_optimizer(cfg, model)
        model.train()
        out.append((model, opt))
    return out, JointsMSELoss(True)


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
    heads = model(x)
    heads = heads if isinstance(heads, list) else [heads]
    loss = None
    for head in heads:                       # what StepGraph sums
        term = crit(head, t, w)
        loss = term if loss is None else loss + term
    opt.zero_grad()
    loss.backward()
    opt.step()
    return heads[-1].detach().clone(), loss.detach().clone()


@pytest.mark.parametrize("kind,streams", [("coam", "single"), ("coam", "engine"), ("transpose", "single")])
def test_fresh_mask_replays_equal_eager_steps_bit_for_bit(dev, kind, streams):
    from buctd_amd import engine, ops
    cfg = _coam_cfg() if kind == "coam" else _transpose_cfg()
    ((eager, eopt), (graphed, gopt)), crit = _engines(kind, cfg, dev)
    sizes = [2, 2, 2, 2, 1, 2, 2]            # warm-up, warm-up, capture + replay, replay, ragged eager batch, replays
    batches = [_batch(cfg, n, 700 + i, dev) for i, n in enumerate(sizes)]
    ops.manual_seed(SEED)
    ref = [_eager_step(eager, eopt, crit, *b) for b in batches]
    drawn_e = ops.seeds_drawn()
    assert drawn_e > 0                       # the model draws masks
    ops.manual_seed(SEED)
    ops.set_grad_arena(gopt.flat)
    step = engine.StepGraph(graphed, crit, gopt, warmup=2, streams=streams, fresh_dropout_masks=True)
    for i, b in enumerate(batches):
        ops.set_grad_arena(gopt.flat)
        out, loss = step(*b)
        assert torch.equal(loss.detach(), ref[i][1]), (i, float(loss), float(ref[i][1]))
        assert torch.equal(out.detach(), ref[i][0]), i
    assert step.replays == 4
    assert ops.seeds_drawn() == drawn_e
    assert torch.equal(eopt.flat.flat, gopt.flat.flat)
    assert torch.equal(eopt.exp_avg, gopt.exp_avg) and torch.equal(eopt.exp_avg_sq, gopt.exp_avg_sq)
    sd_e, sd_g = eager.module.state_dict(), graphed.module.state_dict()
    for k in sd_e:
        assert torch.equal(sd_e[k], sd_g[k]), k


def test_two_replays_of_one_batch_draw_different_masks(dev):
    """learning rate 0: the parameters stay put, so two replays on the same batch differ by their masks alone - and each
    equals its eager twin"""
    from buctd_amd import engine, ops
    cfg = _coam_cfg(lr=0.0)
    ((eager, eopt), (graphed, gopt)), crit = _engines("coam", cfg, dev)
    x, t, w = _batch(cfg, 2, 900, dev)
    ops.manual_seed(SEED)
    ref = [_eager_step(eager, eopt, crit, x, t, w) for _ in range(3)]
    ops.manual_seed(SEED)
    step = engine.StepGraph(graphed, crit, gopt, warmup=1, fresh_dropout_masks=True)
    got = []
    for _ in range(3):
        ops.set_grad_arena(gopt.flat)
        out, loss = step(x, t, w)
        got.append((out.detach().clone(), loss.detach().clone()))
    assert step.replays == 2
    assert not torch.equal(got[1][0], got[2][0])
    for (oe, le), (og, lg) in zip(ref, got):
        assert torch.equal(oe, og) and torch.equal(le, lg)


def test_train_entry_point_with_fresh_masks_logs_the_eager_losses(dev):
    from buctd_amd import engine, ops
    from buctd_amd.core.function import train
    cfg = _coam_cfg()
    ((eager, eopt), (graphed, gopt)), crit = _engines("coam", cfg, dev)
    loader = [(*_batch(cfg, 2, 500 + i, torch.device("cpu")), {}) for i in range(5)]

    class Writer:
        def __init__(self):
            self.losses = []

        def add_scalar(self, k, v, s):
            if k == "train_loss":
                self.losses.append(float(v))

    c = cfg.clone()
    c.defrost()
    c.PRINT_FREQ = 1
    c.freeze()
    we, wg = {"writer": Writer(), "train_global_steps": 0}, {"writer": Writer(), "train_global_steps": 0}
    ops.manual_seed(SEED)
    ops.set_grad_arena(eopt.flat)
    train(c, loader, eager, crit, eopt, 0, "/tmp", "/tmp", we)
    ops.manual_seed(SEED)
    ops.set_grad_arena(gopt.flat)
    step = engine.StepGraph(graphed, crit, gopt, warmup=1, fresh_dropout_masks=True)
    train(c, loader, graphed, crit, gopt, 0, "/tmp", "/tmp", wg, step_graph=step)
    assert step.replays == 4
    assert we["writer"].losses == wg["writer"].losses
    assert torch.equal(eopt.flat.flat, gopt.flat.flat)


def test_both_dropout_keywords_are_refused(dev):
    from buctd_amd import engine
    cfg = _coam_cfg()
    ((model, opt),), crit = _engines("coam", cfg, dev, n=1)
    with pytest.raises(ValueError):
        engine.StepGraph(model, crit, opt, allow_repeated_dropout_masks=True, fresh_dropout_masks=True)


@pytest.mark.parametrize("mode", ["fresh", "repeated"])
def test_a_failed_capture_leaves_batch_and_seed_counts_as_they_were(dev, mode):
    from buctd_amd import engine, ops
    from buctd_amd.core.loss import JointsMSELoss
    cfg = _coam_cfg()
    ((model, opt),), _ = _engines("coam", cfg, dev, n=1)
    inner = JointsMSELoss(True)

    def crit(out, t, w):
        if ops.capturing():
            raise RuntimeError("forced capture failure")
        return inner(out, t, w)

    kw = {"fresh_dropout_masks": True} if mode == "fresh" else {"allow_repeated_dropout_masks": True}
    step = engine.StepGraph(model, crit, opt, warmup=1, **kw)
    ops.manual_seed(SEED)
    ops.set_grad_arena(opt.flat)
    x, t, w = _batch(cfg, 2, 950, dev)
    step(x, t, w)                            # warm-up: an eager step
    tracked = {k: int(v) for k, v in model.module.state_dict().items() if k.endswith("num_batches_tracked")}
    drawn = ops.seeds_drawn()
    with pytest.raises(RuntimeError, match="forced capture failure"):
        step(x, t, w)
    assert not ops.capturing()
    assert ops.seeds_drawn() == drawn
    after = {k: int(v) for k, v in model.module.state_dict().items() if k.endswith("num_batches_tracked")}
    assert after == tracked
    # the eager engine stays usable, and counts on from where it was
    out, loss = _eager_step(model, opt, inner, x, t, w)
    assert torch.isfinite(loss)
    assert ops.seeds_drawn() > drawn
