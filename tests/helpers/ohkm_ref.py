"""fp64 numpy restatement of JointsOHKMMSELoss (reference lib/core/loss.py:140-182) with its gradient, the case table of
tests/golden/ohkm_loss.npz and the input generators shared by the host and the GPU test of the OHKM loss.

    l[n][k] = 0.5/HW * w[n][k]^2 * sum_hw (pred - gt)^2          (loss.py:166-179: 0.5 * MSE(reduction none), mean over HW)
    S_n     = the topk joints of sample n with the largest l      (loss.py:151-153)
    loss    = 1/(N*topk) * sum_n sum_{k in S_n} l[n][k]           (loss.py:154-156)
    grad    = [k in S_n] * w^2 (pred - gt) / (HW*N*topk)

Ties go to the lower joint index (a stable descending sort) - the rule of buctd_joints_ohkm_mse."""
import numpy as np

# (name, N, K, H, W, topk): the shapes of tests/golden/ohkm_loss.npz.  "zerow" has weight 0 on more than K - topk joints of
# every sample, so zero-loss joints are selected: they carry zero gradient, the result does not depend on which.
GOLDEN_CASES = [
    ("a", 4, 17, 16, 12, 8),
    ("b", 3, 14, 8, 6, 14),
    ("c", 2, 17, 64, 48, 1),
    ("zerow", 2, 17, 16, 12, 8),
]
# Case "c" is 2 x 17 x 64 x 48: its inputs are not stored, they are the legacy (frozen) numpy RandomState stream of this
# seed, pinned in the file by their float64 sums.
SEEDED_INPUTS = {"c": 20240603}


def seeded_inputs(seed, n, k, h, w):
    """pred, gt, weight of a golden case whose inputs are regenerated instead of stored."""
    rs = np.random.RandomState(seed)
    pred = rs.standard_normal((n, k, h, w)).astype(np.float32)
    gt = rs.random_sample((n, k, h, w)).astype(np.float32)
    wt = (0.25 + 0.75 * rs.random_sample((n, k, 1))).astype(np.float32)
    return pred, gt, wt


def golden_case(gold, name, n, k, h, w):
    """pred, gt, wt of a case of the golden file (regenerated and checked against its pinned sums where not stored)."""
    if name in SEEDED_INPUTS:
        assert int(gold[f"{name}_seed"]) == SEEDED_INPUTS[name]
        pred, gt, wt = seeded_inputs(SEEDED_INPUTS[name], n, k, h, w)
        assert pred.astype(np.float64).sum() == float(gold[f"{name}_pred_sum"])
        assert gt.astype(np.float64).sum() == float(gold[f"{name}_gt_sum"])
        assert np.array_equal(wt, gold[f"{name}_wt"])
        return pred, gt, wt
    return gold[f"{name}_pred"], gold[f"{name}_gt"], gold[f"{name}_wt"]


def random_inputs(seed, n, k, h, w, zero_fraction=0.3):
    """Continuous random heat-maps and weights (some exactly 0) for the larger GPU shapes.  Every joint's prediction has
    an amplitude of its own: identically distributed rows of thousands of pixels would all have nearly the same loss."""
    rs = np.random.RandomState(seed)
    amp = (0.5 + 1.5 * rs.random_sample((n, k, 1, 1))).astype(np.float32)
    pred = amp * rs.standard_normal((n, k, h, w)).astype(np.float32)
    gt = rs.random_sample((n, k, h, w)).astype(np.float32)
    wt = ((rs.random_sample((n, k, 1)) > zero_fraction) * (0.1 + 0.9 * rs.random_sample((n, k, 1)))).astype(np.float32)
    return pred, gt, wt


def per_joint_loss(pred, gt, wt):
    """[N, K] float64; wt None: no target weight."""
    n, k = pred.shape[:2]
    d = pred.reshape(n, k, -1).astype(np.float64) - gt.reshape(n, k, -1).astype(np.float64)
    w2 = np.ones((n, k)) if wt is None else wt.reshape(n, k).astype(np.float64) ** 2
    return 0.5 * w2 * (d * d).mean(axis=2)


def select(l, topk):
    """[N, K] bool: the topk largest of each row, ties to the lower index."""
    order = np.argsort(-l, axis=1, kind="stable")
    sel = np.zeros(l.shape, dtype=bool)
    np.put_along_axis(sel, order[:, :topk], True, axis=1)
    return sel


def ohkm(pred, gt, wt, topk):
    """-> (loss, grad [N, K, H, W], selected [N, K]) in float64"""
    n, k = pred.shape[:2]
    hw = pred[0, 0].size
    l = per_joint_loss(pred, gt, wt)
    sel = select(l, topk)
    loss = (l * sel).sum() / (n * topk)
    w2 = np.ones((n, k)) if wt is None else wt.reshape(n, k).astype(np.float64) ** 2
    coef = sel * w2 / (hw * n * topk)
    grad = coef.reshape(n, k, *([1] * (pred.ndim - 2))) * (pred.astype(np.float64) - gt.astype(np.float64))
    return loss, grad, sel


def selection_gap_ok(l, topk, rel=1e-4):
    """The condition under which an fp32 and an fp64 evaluation select the same joints, or differ only where it cannot
    show: in every sample the topk-th and (topk+1)-th largest loss are at least `rel` (relative) apart - or the topk-th is
    exactly 0, where every candidate for the remaining places has loss 0 and gradient 0.  topk == K: nothing to separate."""
    k = l.shape[1]
    if topk >= k:
        return True
    s = -np.sort(-l, axis=1)
    a, b = s[:, topk - 1], s[:, topk]
    return bool(np.all((a - b >= rel * a) & (a > 0) | (a == 0)))
