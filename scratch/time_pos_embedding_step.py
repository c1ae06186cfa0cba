"""usage: time_pos_embedding_step.py ROOT PE STEPS OUT.jsonl : the eager train step of TransPose-H-A6 256x192 at batch 8
(FusedAdam) with MODEL.POS_EMBEDDING = PE (sine | learnable | none), imported from the checkout ROOT (this one: `.`; a built
checkout of another commit to compare against); appends one JSON line.  Alternate the calls of the variants compared."""
import json
import os
import statistics
import sys
import time

root, pe, steps, out = os.path.abspath(sys.argv[1]), sys.argv[2], int(sys.argv[3]), sys.argv[4]
sys.path.insert(0, root)
import torch  # noqa: E402

import buctd_amd  # noqa: E402
from buctd_amd import engine, models  # noqa: E402
from buctd_amd.config import cfg as base, hrnet_extra  # noqa: E402
from buctd_amd.core.loss import JointsMSELoss  # noqa: E402

assert os.path.abspath(buctd_amd.__file__).startswith(root), buctd_amd.__file__
BATCH = 8
c = base.clone()
c.defrost()
c.MODEL.NAME = "transpose_h"
c.MODEL.NUM_JOINTS = 17
c.MODEL.IMAGE_SIZE = [192, 256]
c.MODEL.HEATMAP_SIZE = [48, 64]
c.MODEL.SIGMA = 2
c.MODEL.PRETRAINED = ""
c.MODEL.CONDITIONAL_TOPDOWN = True
c.MODEL.EXTRA = hrnet_extra(48, use_attention=True)
c.MODEL.POS_EMBEDDING = pe
c.DATASET.DATASET = "coco"
c.DATASET.COLORED = True
c.freeze()
dev = torch.device("cuda:0")
torch.manual_seed(1234)
net = models.transpose_h.get_pose_net(c, is_train=True).to(dev)
model = engine.DataParallel(net)
opt = engine.get_optimizer(c, model)
model.train()
g = torch.Generator().manual_seed(7)
x = torch.randn(BATCH, 6, 256, 192, generator=g).to(dev)
t = torch.rand(BATCH, 17, 64, 48, generator=g).to(dev)
w = torch.ones(BATCH, 17, 1).to(dev)
crit = JointsMSELoss(True)


def step():
    loss = crit(model(x), t, w)
    opt.zero_grad()
    loss.backward()
    opt.step()
    return loss


for _ in range(6):
    step()
torch.cuda.synchronize()
times = []
load0 = os.getloadavg()[0]
for _ in range(steps):
    t0 = time.perf_counter()
    loss = step()
    torch.cuda.synchronize()
    times.append((time.perf_counter() - t0) * 1e3)
res = {"tree": os.path.basename(root) or "current", "pos_embedding": pe, "batch": BATCH, "steps": steps,
       "step_ms_median": statistics.median(times), "step_ms_min": min(times), "step_ms_max": max(times),
       "loss": float(loss.detach()), "load_1min": [load0, os.getloadavg()[0]]}
print(json.dumps(res), flush=True)
with open(out, "a") as f:
    f.write(json.dumps(res) + "\n")
