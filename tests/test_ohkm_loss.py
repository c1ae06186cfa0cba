"""JointsOHKMMSELoss, host side (no GPU): the criterion a config selects, the reference's constructor, the C ABI of the two
new entry points, and the fp64 restatement the GPU test compares the kernels with (tests/helpers/ohkm_ref.py) against the
reference's own outputs in tests/golden/ohkm_loss.npz (written by scratch/make_ohkm_golden.py from the reference class,
lib/core/loss.py:140-182, on the CPU)."""
import inspect
import os

import numpy as np
import pytest

from tests.helpers import ohkm_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ohkm_loss.npz")


def golden_modes(name):
    return ("w",) if name == "zerow" else ("w", "nw")


def test_get_criterion_follows_use_ohkm():
    from buctd_amd.config import cfg as base
    from buctd_amd.core.loss import JointsMSELoss, JointsOHKMMSELoss, get_criterion
    c = base.clone()
    c.defrost()
    c.LOSS.USE_OHKM = False
    c.LOSS.USE_TARGET_WEIGHT = False
    crit = get_criterion(c)
    assert type(crit) is JointsMSELoss and crit.use_target_weight is False
    c.LOSS.USE_OHKM = True
    c.LOSS.USE_TARGET_WEIGHT = True
    c.LOSS.TOPK = 5
    crit = get_criterion(c)
    assert type(crit) is JointsOHKMMSELoss and crit.use_target_weight is True and crit.topk == 5
    # the default config keeps the plain loss
    assert type(get_criterion(base)) is JointsMSELoss


def test_constructor_and_forward_signatures_equal_the_reference():
    """reference lib/core/loss.py:141 `__init__(self, use_target_weight, topk=8)`, :159 `forward(self, output, target,
    target_weight)`"""
    from buctd_amd.core.loss import JointsOHKMMSELoss
    sig = inspect.signature(JointsOHKMMSELoss.__init__)
    assert list(sig.parameters) == ["self", "use_target_weight", "topk"]
    assert sig.parameters["use_target_weight"].default is inspect.Parameter.empty
    assert sig.parameters["topk"].default == 8
    assert list(inspect.signature(JointsOHKMMSELoss.forward).parameters) == ["self", "output", "target", "target_weight"]
    crit = JointsOHKMMSELoss(True)
    assert crit.topk == 8 and crit.use_target_weight is True


def test_the_criterion_refuses_cpu_tensors():
    import torch
    from buctd_amd.core.loss import JointsOHKMMSELoss
    with pytest.raises(RuntimeError, match="ROCm device only"):
        JointsOHKMMSELoss(True, 2)(torch.zeros(2, 4, 3, 3), torch.zeros(2, 4, 3, 3), torch.ones(2, 4, 1))


def test_c_abi_declares_and_exports_the_two_entry_points():
    import ctypes as C
    from buctd_amd import _C
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "buctd_hip.h")).read()
    for name in ("buctd_joints_ohkm_mse_workspace", "buctd_joints_ohkm_mse"):
        assert name + "(" in header and name in _C.SIGNATURES
        assert getattr(_C.lib(), name) is not None
    res, args = _C.SIGNATURES["buctd_joints_ohkm_mse"]
    assert res is C.c_int and len(args) == 13 and args[-1] is C.c_void_p and args[-2] is C.c_size_t
    # the workspace query is host code: l[N][K] and the gradient scale [N][K]
    assert _C.lib().buctd_joints_ohkm_mse_workspace(32, 17) == 2 * 32 * 17 * 4
    assert "BUCTD_OHKM_MAX_JOINTS 64" in header


@pytest.mark.parametrize("case", R.GOLDEN_CASES, ids=[c[0] for c in R.GOLDEN_CASES])
def test_fp64_restatement_reproduces_the_reference_golden(case):
    name, n, k, h, w, topk = case
    gold = np.load(GOLD)
    assert int(gold[f"{name}_topk"]) == topk
    pred, gt, wt = R.golden_case(gold, name, n, k, h, w)
    assert pred.shape == (n, k, h, w) and n >= 2
    for mode in golden_modes(name):
        weights = wt if mode == "w" else None
        l = R.per_joint_loss(pred, gt, weights)
        assert R.selection_gap_ok(l, topk), "the golden inputs must separate the topk-th from the next joint"
        loss, grad, sel = R.ohkm(pred, gt, weights, topk)
        assert (sel.sum(axis=1) == topk).all()
        ref_loss, ref_grad = float(gold[f"{name}_{mode}_loss"]), gold[f"{name}_{mode}_grad"]
        assert abs(loss - ref_loss) <= 1e-6 * abs(ref_loss), (mode, loss, ref_loss)
        assert np.abs(grad - ref_grad).max() <= 1e-6 * np.abs(ref_grad).max(), mode
        # the reference leaves the joints it did not select without gradient
        assert not ref_grad[~sel].any()


def test_golden_zero_weight_case_selects_zero_loss_joints():
    name, n, k, h, w, topk = R.GOLDEN_CASES[-1]
    gold = np.load(GOLD)
    wt = gold[f"{name}_wt"].reshape(n, k)
    assert name == "zerow" and ((wt == 0).sum(axis=1) > k - topk).all()


def test_restatement_breaks_ties_towards_the_lower_index():
    l = np.array([[1.0, 3.0, 3.0, 0.5, 3.0]])
    assert R.select(l, 2).tolist() == [[False, True, True, False, False]]
    assert R.select(l, 1).tolist() == [[False, True, False, False, False]]
    assert not R.selection_gap_ok(l, 2) and R.selection_gap_ok(l, 3)
