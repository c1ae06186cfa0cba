"""Times the heat-map losses at N = 32, K = 17, 96 x 72 on the MI355X (device events, warm-up, median):
  (a) JointsMSELoss forward + gradient (buctd_joints_mse),
  (b) JointsOHKMMSELoss forward + gradient (buctd_joints_ohkm_mse, topk 8),
  (c) a plain PyTorch-ROCm restatement of the reference loop (lib/core/loss.py:140-182) with autograd.
Each sample is the device time of REPS back-to-back calls between two events, divided by REPS; (a) and (b) are also
replayed from a captured graph of REPS calls, which takes the host's enqueue rate out of the number.

    python scratch/time_ohkm_loss.py [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N, K, H, W, TOPK = 32, 17, 96, 72, 8
REPS, SAMPLES, WARMUP = 20, 30, 5


def torch_ohkm(output, target, target_weight, topk):
    """the reference's loop: per-joint 0.5 * MSE(none) -> mean over pixels -> per-sample topk / gather / sum"""
    n, k = output.size(0), output.size(1)
    pred = output.reshape(n, k, -1).split(1, 1)
    gt = target.reshape(n, k, -1).split(1, 1)
    loss = []
    for idx in range(k):
        p, g = pred[idx].squeeze(1), gt[idx].squeeze(1)
        loss.append(0.5 * F.mse_loss(p.mul(target_weight[:, idx]), g.mul(target_weight[:, idx]), reduction="none"))
    loss = torch.cat([l.mean(dim=1).unsqueeze(dim=1) for l in loss], dim=1)
    total = 0.0
    for i in range(n):
        _, idx = torch.topk(loss[i], k=topk, dim=0, sorted=False)
        total = total + torch.gather(loss[i], 0, idx).sum() / topk
    return total / n


def median_us(fn, reps=REPS):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(SAMPLES):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    return statistics.median(out), min(out), max(out)


def graphed(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(REPS):
            fn()
    return g.replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from buctd_amd import ops
    from buctd_amd.core.loss import JointsMSELoss, JointsOHKMMSELoss
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    pred = (torch.randn(N, K, H, W, generator=g) * (0.5 + torch.rand(N, K, 1, 1, generator=g))).to(dev)
    gt = torch.rand(N, K, H, W, generator=g).to(dev)
    w = torch.rand(N, K, generator=g).to(dev)
    w3 = w.reshape(N, K, 1)

    def module_step(crit):
        def run():
            p = pred.detach().requires_grad_(True)
            crit(p, gt, w3).backward()
        return run

    def torch_step():
        p = pred.detach().requires_grad_(True)
        torch_ohkm(p, gt, w3, TOPK).backward()

    res = {"shape": {"N": N, "K": K, "H": H, "W": W, "topk": TOPK}, "reps_per_sample": REPS, "samples": SAMPLES,
           "unit": "us per call: median [min, max] of the samples", "device": torch.cuda.get_device_name(0)}
    rows = [
        ("a_joints_mse_kernels", lambda: ops.joints_mse(pred, gt, w, True), True),
        ("b_joints_ohkm_mse_kernels", lambda: ops.joints_ohkm_mse(pred, gt, w, TOPK, True), True),
        ("a_JointsMSELoss_forward_backward", module_step(JointsMSELoss(True)), False),
        ("b_JointsOHKMMSELoss_forward_backward", module_step(JointsOHKMMSELoss(True, TOPK)), False),
        ("c_torch_restatement_forward_backward", torch_step, False),
    ]
    for name, fn, graph in rows:
        med, lo, hi = median_us(fn)
        res[name] = {"eager": [round(med, 2), round(lo, 2), round(hi, 2)]}
        if graph:
            try:
                med, lo, hi = median_us(graphed(fn), reps=1)
                res[name]["graph_replay"] = [round(med / REPS, 2), round(lo / REPS, 2), round(hi / REPS, 2)]
            except RuntimeError as e:      # the eager numbers stand on their own
                res[name]["graph_replay_error"] = str(e)[:200]
        print(name, res[name], flush=True)
    # sanity: the restatement and the kernel agree on what is being timed
    p = pred.detach().requires_grad_(True)
    ref = torch_ohkm(p, gt, w3, TOPK)
    got, _ = ops.joints_ohkm_mse(pred, gt, w, TOPK, False)
    res["loss_kernel_vs_torch"] = [float(got), float(ref.detach())]
    assert abs(float(got) - float(ref.detach())) <= 1e-5 * abs(float(ref.detach())), res["loss_kernel_vs_torch"]
    bytes_rows = 2 * pred.numel() * 4
    res["bytes"] = {"a": bytes_rows + pred.numel() * 4, "b_selected_only": bytes_rows + (bytes_rows * TOPK // K) + pred.numel() * 4}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
