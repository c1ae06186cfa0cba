"""Writes tests/golden/ohkm_loss.npz: inputs and outputs of the reference's own JointsOHKMMSELoss (lib/core/loss.py:140-182),
imported from a reference checkout and run on the CPU - loss and output.grad from autograd, with and without the target
weight, on the shapes of tests/helpers/ohkm_ref.py.  Only data is kept; nothing of the reference's sources is copied.

    python scratch/make_ohkm_golden.py --reference <checkout of the reference> [--out tests/golden/ohkm_loss.npz]

Keys per case <c> of GOLDEN_CASES: <c>_pred, <c>_gt, <c>_wt (or <c>_seed, <c>_pred_sum, <c>_gt_sum for a case whose inputs are
regenerated from a seed), <c>_topk, and per weight mode m in (w, nw): <c>_<m>_loss, <c>_<m>_grad."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.helpers import ohkm_ref as R  # noqa: E402


def inputs(name, n, k, h, w, topk):
    if name in R.SEEDED_INPUTS:
        return R.seeded_inputs(R.SEEDED_INPUTS[name], n, k, h, w)
    rs = np.random.RandomState(1000 + sum(map(ord, name)))
    pred = rs.standard_normal((n, k, h, w)).astype(np.float32)
    gt = rs.random_sample((n, k, h, w)).astype(np.float32)
    wt = (0.25 + 0.75 * rs.random_sample((n, k, 1))).astype(np.float32)
    if name == "zerow":
        # more than K - topk joints of every sample get weight 0: fewer than topk joints have a non-zero loss
        for i in range(n):
            zero = rs.permutation(k)[:k - topk + 3 + i]
            wt[i, zero] = 0.0
    return pred, gt, wt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ohkm_loss.npz"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(a.reference, "lib"))
    from core.loss import JointsOHKMMSELoss  # the reference class

    out = {}
    for name, n, k, h, w, topk in R.GOLDEN_CASES:
        pred, gt, wt = inputs(name, n, k, h, w, topk)
        if name in R.SEEDED_INPUTS:
            out[f"{name}_seed"] = np.int64(R.SEEDED_INPUTS[name])
            out[f"{name}_pred_sum"] = pred.astype(np.float64).sum()
            out[f"{name}_gt_sum"] = gt.astype(np.float64).sum()
        else:
            out[f"{name}_pred"], out[f"{name}_gt"] = pred, gt
        out[f"{name}_wt"] = wt
        out[f"{name}_topk"] = np.int64(topk)
        for mode, use_w in (("w", True), ("nw", False)):
            if name == "zerow" and not use_w:
                continue
            p = torch.from_numpy(pred).clone().requires_grad_(True)
            loss = JointsOHKMMSELoss(use_w, topk)(p, torch.from_numpy(gt), torch.from_numpy(wt))
            loss.backward()
            out[f"{name}_{mode}_loss"] = loss.detach().numpy()
            out[f"{name}_{mode}_grad"] = p.grad.numpy()
            # the restatement agrees before anything is written
            l64, g64, _ = R.ohkm(pred, gt, wt if use_w else None, topk)
            assert R.selection_gap_ok(R.per_joint_loss(pred, gt, wt if use_w else None), topk), (name, mode)
            assert abs(float(loss.detach()) - l64) <= 1e-6 * abs(l64), (name, mode, float(loss.detach()), l64)
            assert np.abs(p.grad.numpy() - g64).max() <= 1e-6 * np.abs(g64).max(), (name, mode)
            print(f"{name}/{mode}: loss {float(loss.detach()):.8f}  restatement {l64:.8f}")
    np.savez_compressed(a.out, **out)
    print(f"wrote {a.out}: {os.path.getsize(a.out) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
