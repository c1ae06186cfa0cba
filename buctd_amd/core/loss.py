"""JointsMSELoss and JointsOHKMMSELoss on the MI355X engine - drop-ins for reference lib/core/loss.py:17-41 and 140-182.

The reference loops over the K joints in Python and launches 3 small kernels per joint; here one fused
kernel computes 0.5/(K*N*HW) * sum w^2 (pred-gt)^2 and its gradient in a single pass over the heat-maps.
The OHKM loss (online hard key-point mining: per sample, only the topk joints with the largest loss count) adds a
per-sample torch.topk / gather to that loop; here the selection runs on the device between two passes over the
heat-maps, so the criterion reads nothing back to the host and a captured step re-selects on every replay.
"""
import torch

from .. import ops


class JointsMSELoss(torch.nn.Module):
    def __init__(self, use_target_weight):
        super().__init__()
        self.use_target_weight = use_target_weight

    def forward(self, output, target, target_weight):
        if not output.is_cuda:
            raise RuntimeError("buctd_amd JointsMSELoss runs on the ROCm device only")
        n, k = output.size(0), output.size(1)
        out = output.contiguous()
        tgt = target.to(out.device, torch.float32).contiguous()
        w = None
        if self.use_target_weight:
            w = target_weight.to(out.device, torch.float32).reshape(n, k).contiguous()
        return ops.JointsMSE.apply(out, tgt, w)


class JointsOHKMMSELoss(torch.nn.Module):
    def __init__(self, use_target_weight, topk=8):
        super().__init__()
        self.use_target_weight = use_target_weight
        self.topk = topk

    def forward(self, output, target, target_weight):
        if not output.is_cuda:
            raise RuntimeError("buctd_amd JointsOHKMMSELoss runs on the ROCm device only")
        n, k = output.size(0), output.size(1)
        out = output.contiguous()
        tgt = target.to(out.device, torch.float32).contiguous()
        w = None
        if self.use_target_weight:
            w = target_weight.to(out.device, torch.float32).reshape(n, k).contiguous()
        return ops.JointsOHKMMSE.apply(out, tgt, w, self.topk)


def get_criterion(cfg):
    """The training criterion a config asks for: LOSS.USE_OHKM selects JointsOHKMMSELoss(LOSS.TOPK)."""
    if cfg.LOSS.USE_OHKM:
        return JointsOHKMMSELoss(cfg.LOSS.USE_TARGET_WEIGHT, cfg.LOSS.TOPK)
    return JointsMSELoss(cfg.LOSS.USE_TARGET_WEIGHT)
