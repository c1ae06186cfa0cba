"""JointsOHKMMSELoss on the MI355X (buctd_joints_ohkm_mse, csrc/loss_decode.hip) against the fp64 restatement of
tests/helpers/ohkm_ref.py and against the reference's own outputs (tests/golden/ohkm_loss.npz; reference
lib/core/loss.py:140-182).

Bounds: those of the JointsMSELoss test against the reference (test_gpu_core_golden.py,
test_joints_mse_matches_reference_loss_and_gradient): |loss - ref| <= 2e-7 * max(1, |ref|), max |grad - ref| <= 1e-9.
Gradient rows of joints that were not selected must be exactly 0.

The inputs are continuous random values; every case asserts in fp64 that the topk-th and the (topk+1)-th largest per-joint
loss of each sample are at least 1e-4 (relative) apart - or that the topk-th is exactly 0, where the remaining places go
to joints with loss 0 and gradient 0 - so the fp32 kernels and the fp64 restatement select the same joints."""
import os

import numpy as np
import pytest
import torch

from tests.helpers import ohkm_ref as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ohkm_loss.npz")

LOSS_TOL = 2e-7      # * max(1, |ref|)
GRAD_TOL = 1e-9      # absolute


def check(loss, grad, ref_loss, ref_grad, sel, what):
    loss, grad = float(loss), grad.detach().cpu().numpy()
    dl, dg = abs(loss - ref_loss), np.abs(grad - ref_grad).max()
    print(f"{what}: loss {loss:.9f} ref {ref_loss:.9f} |d| {dl:.2e}   grad max|d| {dg:.2e} (max|ref| {np.abs(ref_grad).max():.2e})")
    assert dl <= LOSS_TOL * max(1.0, abs(ref_loss)), (what, loss, ref_loss)
    assert dg <= GRAD_TOL, (what, dg)
    if sel is not None:
        assert not grad[~sel].any(), f"{what}: gradient on a joint that was not selected"


def topks(k):
    return sorted({1, max(1, k // 2), k})


def on_device(dev, *arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


@pytest.mark.parametrize("case", R.GOLDEN_CASES, ids=[c[0] for c in R.GOLDEN_CASES])
def test_kernel_and_module_match_fp64_and_the_reference_on_the_golden_cases(dev, case):
    from buctd_amd import ops
    from buctd_amd.core.loss import JointsOHKMMSELoss
    name, n, k, h, w, topk = case
    gold = np.load(GOLD)
    pred, gt, wt = R.golden_case(gold, name, n, k, h, w)
    modes = ("w",) if name == "zerow" else ("w", "nw")
    for mode in modes:
        weights = wt if mode == "w" else None
        assert R.selection_gap_ok(R.per_joint_loss(pred, gt, weights), topk)
        ref_loss, ref_grad, sel = R.ohkm(pred, gt, weights, topk)
        p, g, wd = on_device(dev, pred, gt, None if weights is None else weights.reshape(n, k))
        loss, grad = ops.joints_ohkm_mse(p, g, wd, topk, True)
        check(loss, grad, ref_loss, ref_grad, sel, f"{name}/{mode} kernel vs fp64")
        # the module (autograd) form the training loop uses, against the reference's own loss and output.grad
        pm = p.clone().requires_grad_(True)
        out = JointsOHKMMSELoss(mode == "w", topk)(pm, g, torch.from_numpy(wt).to(dev))
        out.backward()
        check(out.detach(), pm.grad, float(gold[f"{name}_{mode}_loss"]), gold[f"{name}_{mode}_grad"], sel,
              f"{name}/{mode} module vs reference golden")
        # without a gradient: the same loss from two launches
        loss_only, none = ops.joints_ohkm_mse(p, g, wd, topk, False)
        assert none is None and torch.equal(loss_only, loss)


LARGE = [(h, w, k) for (h, w) in ((96, 72), (64, 48), (15, 11)) for k in (1, 14, 17, 64)]


def large_inputs(h, w, k):
    # seeds under which every (topk, weights) combination below meets the fp64 gap condition (checked without a device)
    return R.random_inputs(8000 + 97 * h + 13 * w + k, 32, k, h, w)


@pytest.mark.parametrize("h,w,k", LARGE, ids=[f"{h}x{w}-K{k}" for h, w, k in LARGE])
def test_kernel_matches_fp64_on_batch_32(dev, h, w, k):
    from buctd_amd import ops
    n = 32
    pred, gt, wt = large_inputs(h, w, k)
    p, g, wd = on_device(dev, pred, gt, wt.reshape(n, k))
    for weights, wdev in ((wt, wd), (None, None)):
        l = R.per_joint_loss(pred, gt, weights)
        for topk in topks(k):
            assert R.selection_gap_ok(l, topk), (h, w, k, topk, weights is not None)
            ref_loss, ref_grad, sel = R.ohkm(pred, gt, weights, topk)
            loss, grad = ops.joints_ohkm_mse(p, g, wdev, topk, True)
            check(loss, grad, ref_loss, ref_grad, sel, f"N32 {h}x{w} K{k} topk{topk} {'w' if weights is not None else 'nw'}")
            assert int((grad.flatten(2).abs().amax(2) > 0).sum(1).max()) <= topk


def test_unaligned_views_take_the_scalar_path(dev):
    """Heat-maps whose storage does not start on 16 bytes (a view at an odd element offset) give the same result."""
    from buctd_amd import ops
    n, k, h, w, topk = 3, 17, 16, 12, 8
    pred, gt, wt = R.random_inputs(4242, n, k, h, w)
    ref_loss, ref_grad, sel = R.ohkm(pred, gt, wt, topk)
    assert R.selection_gap_ok(R.per_joint_loss(pred, gt, wt), topk)
    p, g, wd = on_device(dev, pred, gt, wt.reshape(n, k))
    flat = torch.empty(p.numel() + 1, device=dev)
    pv = flat[1:].view_as(p)
    pv.copy_(p)
    assert pv.data_ptr() % 16 == 4 and pv.is_contiguous()
    loss, grad = ops.joints_ohkm_mse(pv, g, wd, topk, True)
    check(loss, grad, ref_loss, ref_grad, sel, "unaligned pred")
    loss_a, grad_a = ops.joints_ohkm_mse(p, g, wd, topk, True)
    assert torch.equal(grad, grad_a) and abs(float(loss) - float(loss_a)) <= LOSS_TOL


def test_exact_ties_go_to_the_lower_joint_index(dev):
    """Two joints with identical heat-map rows (prediction, target and weight) straddle the cut: the lower index gets the
    gradient, the higher one exact zeros.  The loss does not depend on the rule."""
    from buctd_amd import ops
    n, k, h, w, topk = 2, 6, 16, 12, 3
    rs = np.random.RandomState(5)
    gt = rs.random_sample((n, k, h, w)).astype(np.float32)
    noise = rs.standard_normal((n, k, h, w)).astype(np.float32)
    amp = np.array([[3.0, 2.0, 1.0, 0.5, 1.0, 0.2],        # sample 0: joints 2 and 4 tie for the third place
                    [1.0, 0.2, 3.0, 2.0, 0.5, 1.0]],       # sample 1: joints 0 and 5
                   dtype=np.float32).reshape(n, k, 1, 1)
    pairs = [(2, 4), (0, 5)]
    for i, (lo, hi) in enumerate(pairs):
        gt[i, hi] = gt[i, lo]
        noise[i, hi] = noise[i, lo]
    pred = gt + amp * noise
    wt = np.full((n, k), 0.75, dtype=np.float32)
    l = R.per_joint_loss(pred, gt, wt)
    for i, (lo, hi) in enumerate(pairs):
        assert l[i, lo] == l[i, hi] and (l[i] > l[i, lo]).sum() == topk - 1, "the tied pair must straddle the cut"
    ref_loss, ref_grad, sel = R.ohkm(pred, gt, wt, topk)
    p, g, wd = on_device(dev, pred, gt, wt)
    loss, grad = ops.joints_ohkm_mse(p, g, wd, topk, True)
    check(loss, grad, ref_loss, ref_grad, sel, "ties")
    gnp = grad.cpu().numpy()
    for i, (lo, hi) in enumerate(pairs):
        assert gnp[i, lo].any() and not gnp[i, hi].any(), (i, lo, hi)
        assert sel[i, lo] and not sel[i, hi]


@pytest.mark.parametrize("weighted", [True, False])
def test_topk_equal_to_k_is_the_plain_joints_mse(dev, weighted):
    """For topk = K the formula reduces to JointsMSELoss: 1/(N*K) * sum_n sum_k l[n][k]."""
    from buctd_amd.core.loss import JointsMSELoss, JointsOHKMMSELoss
    n, k, h, w = 32, 17, 64, 48
    pred, gt, wt = R.random_inputs(99, n, k, h, w)
    p, g, wd = on_device(dev, pred, gt, wt)
    pa, pb = p.clone().requires_grad_(True), p.clone().requires_grad_(True)
    la = JointsMSELoss(weighted)(pa, g, wd)
    lb = JointsOHKMMSELoss(weighted, topk=k)(pb, g, wd)
    la.backward()
    lb.backward()
    la, lb = la.detach(), lb.detach()
    dl, dg = abs(float(la) - float(lb)), float((pa.grad - pb.grad).abs().max())
    print(f"topk=K weighted={weighted}: mse {float(la):.9f} ohkm {float(lb):.9f} |d| {dl:.2e}  grad max|d| {dg:.2e}")
    assert dl <= LOSS_TOL * max(1.0, abs(float(la)))
    assert dg <= GRAD_TOL


def test_argument_errors_launch_nothing(dev):
    from buctd_amd import ops
    from buctd_amd._C import BuctdHipError, lib, ptr, stream_ptr
    n, k, h, w = 2, 17, 8, 6
    p = torch.randn(n, k, h, w, device=dev)
    g = torch.rand(n, k, h, w, device=dev)
    with pytest.raises(BuctdHipError, match=r"topk = 0 is outside 1\.\.K = 17"):
        ops.joints_ohkm_mse(p, g, None, 0, True)
    with pytest.raises(BuctdHipError, match=r"topk = 18 is outside 1\.\.K = 17"):
        ops.joints_ohkm_mse(p, g, None, 18, True)
    p65 = torch.randn(2, 65, 4, 4, device=dev)
    with pytest.raises(BuctdHipError, match=r"K = 65 exceeds the limit of 64 joints"):
        ops.joints_ohkm_mse(p65, p65, None, 8, True)
    # a short workspace, at the C entry point; the outputs keep their sentinels: nothing ran
    need = lib().buctd_joints_ohkm_mse_workspace(n, k)
    assert need == 2 * n * k * 4
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    loss = torch.full((), -7.0, device=dev)
    grad = torch.full_like(p, -7.0)
    rc = lib().buctd_joints_ohkm_mse(ptr(p), ptr(g), None, n, k, h * w, 8, ptr(loss), ptr(grad), 1.0, ptr(ws), need - 1,
                                     stream_ptr())
    assert rc == -3 and f"workspace {need - 1} bytes < required {need}" in lib().buctd_last_error().decode()
    rc = lib().buctd_joints_ohkm_mse(ptr(p), ptr(g), None, n, k, h * w, 0, ptr(loss), ptr(grad), 1.0, ptr(ws), need,
                                     stream_ptr())
    assert rc == -1
    torch.cuda.synchronize()
    assert float(loss) == -7.0 and bool((grad == -7.0).all())
    # the same buffers with valid arguments: the call goes through
    rc = lib().buctd_joints_ohkm_mse(ptr(p), ptr(g), None, n, k, h * w, 8, ptr(loss), ptr(grad), 1.0, ptr(ws), need,
                                     stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    assert float(loss) > 0 and int((grad.flatten(2).abs().amax(2) > 0).sum()) == n * 8


def test_step_graph_reselects_on_every_replay(dev):
    """get_criterion(cfg) with LOSS.USE_OHKM under engine.StepGraph (the small preNet HRNet of test_gpu_step_graph.py):
    losses, outputs and parameters equal the eager engine's bit for bit over warm-up, capture and replays, and the joints
    that receive gradient differ between replayed steps - the selection runs on the device in every replay."""
    import copy
    from buctd_amd import engine, models, ops
    from buctd_amd.core.loss import JointsOHKMMSELoss, get_criterion
    from tests.test_gpu_step_graph import _batch, _prenet_cfg
    cfg = _prenet_cfg().clone()
    cfg.defrost()
    cfg.LOSS.USE_OHKM = True
    cfg.LOSS.TOPK = 8
    cfg.freeze()
    crit = get_criterion(cfg)
    assert isinstance(crit, JointsOHKMMSELoss) and crit.topk == 8 and crit.use_target_weight
    torch.manual_seed(7)
    net_a = models.pose_hrnet.get_pose_net(cfg, is_train=True).to(dev)
    net_b = copy.deepcopy(net_a)
    (eager, eopt), (graphed, gopt) = [(m, engine.get_optimizer(cfg, m)) for m in
                                      (engine.DataParallel(net_a), engine.DataParallel(net_b))]
    eager.train()
    graphed.train()
    warmup, steps = 2, 7
    step = engine.StepGraph(graphed, crit, gopt, warmup=warmup)
    selected = []
    for i in range(steps):
        x, t, w = _batch(cfg, 4, 2100 + i, dev)
        engine.ops.set_grad_arena(eopt.flat)
        out_e = eager(x)
        loss_e = crit(out_e, t, w)
        eopt.zero_grad()
        loss_e.backward()
        eopt.step()
        engine.ops.set_grad_arena(gopt.flat)
        out_g, loss_g = step(x, t, w)
        assert torch.equal(loss_e.detach(), loss_g.detach()), (i, float(loss_e), float(loss_g))
        assert torch.equal(out_e.detach(), out_g.detach()), i
        # the joints this step's criterion gave gradient to, from the step's own output
        _, grad = ops.joints_ohkm_mse(out_g.detach().contiguous(), t, w.reshape(4, -1).contiguous(), 8, True)
        selected.append((grad.flatten(2).abs().amax(2) > 0).cpu().numpy())
    assert step.replays == steps - warmup and step.replays >= 4
    replayed = selected[warmup + 1:]          # the steps after the one that captured
    assert len(replayed) >= 3
    assert any(not np.array_equal(replayed[0], s) for s in replayed[1:]), "the selection never changed between replays"
    assert torch.equal(eopt.flat.flat, gopt.flat.flat)
    assert torch.equal(eopt.exp_avg, gopt.exp_avg) and torch.equal(eopt.exp_avg_sq, gopt.exp_avg_sq)
    sd_e, sd_g = eager.module.state_dict(), graphed.module.state_dict()
    for name in sd_e:
        assert torch.equal(sd_e[name], sd_g[name]), name


def test_train_entry_point_runs_with_the_ohkm_criterion(dev):
    """core.function.train takes the criterion as it takes JointsMSELoss (multi-head outputs are summed by the caller)."""
    from buctd_amd import engine, models
    from buctd_amd.core.function import train
    from buctd_amd.core.loss import get_criterion
    from tests.test_gpu_step_graph import _batch, _prenet_cfg
    cfg = _prenet_cfg().clone()
    cfg.defrost()
    cfg.LOSS.USE_OHKM = True
    cfg.LOSS.TOPK = 8
    cfg.PRINT_FREQ = 1
    cfg.freeze()
    torch.manual_seed(11)
    model = engine.DataParallel(models.pose_hrnet.get_pose_net(cfg, is_train=True).to(dev))
    opt = engine.get_optimizer(cfg, model)
    engine.ops.set_grad_arena(opt.flat)
    loader = [(*_batch(cfg, 2, 2300 + i, torch.device("cpu")), {}) for i in range(3)]

    class Writer:
        losses = []

        def add_scalar(self, key, v, s):
            if key == "train_loss":
                self.losses.append(float(v))

    wd = {"writer": Writer(), "train_global_steps": 0}
    before = opt.flat.flat.clone()
    train(cfg, loader, model, get_criterion(cfg), opt, 0, "/tmp", "/tmp", wd)
    assert len(wd["writer"].losses) == 3 and all(np.isfinite(v) and v > 0 for v in wd["writer"].losses)
    assert not torch.equal(before, opt.flat.flat)
