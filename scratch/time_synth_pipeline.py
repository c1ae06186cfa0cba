"""Times one generative-sampling train batch at the headline shape (batch 32, 384 x 288, K = 14 crowdpose, M = 2
neighbours, colored condition) on the MI355X, two ways:
  new   DeviceSamplePipeline(records, aug, seed) with DATASET.SYNTHESIS_POSE: synthesis -> buctd_cond_geometry -> render,
        nothing copied back;
  hand  what a user had to write before: synthesize_pose_batch -> .cpu() -> geometry() per record with the synthesized
        pose as its condition -> render().
Per batch: host time = until the call returns, batch time = until the device is idle (torch.cuda.synchronize);
samples/s = 32 / median batch time.  --tree points at another checkout (with its own built library) to time `hand` on
the commit before the new call existed.

    python scratch/time_synth_pipeline.py --path new|hand [--tree DIR] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

B, K, M, IMG_H, IMG_W = 32, 14, 2, 480, 640
BATCHES, WARMUP = 40, 8
FLIP_PAIRS = [[0, 1], [2, 3], [4, 5], [6, 7], [8, 9], [10, 11]]
COLORS = [[245, 53, 53], [245, 125, 45], [253, 206, 20], [206, 244, 54], [118, 253, 27], [47, 254, 47], [25, 245, 113],
          [15, 243, 197], [14, 199, 245], [44, 126, 249], [13, 13, 249], [128, 47, 249], [205, 38, 247], [245, 48, 206]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--path", choices=["new", "hand"], required=True)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    from buctd_amd.config import cfg as base
    from buctd_amd.dataset.pipeline import DeviceSamplePipeline
    from buctd_amd.dataset.pose_synthesis import synthesize_pose_batch
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    dev = torch.device("cuda:0")
    c = base.clone()
    c.defrost()
    c.MODEL.NUM_JOINTS, c.MODEL.IMAGE_SIZE, c.MODEL.HEATMAP_SIZE, c.MODEL.SIGMA = K, [288, 384], [72, 96], 3
    c.MODEL.CONDITIONAL_TOPDOWN, c.DATASET.COLORED, c.DATASET.DATASET = True, True, "crowdpose"
    c.DATASET.SYNTHESIS_POSE = a.path == "new"
    c.freeze()
    pipe = DeviceSamplePipeline(c, FLIP_PAIRS, range(8), COLORS, is_train=True, seed=0)
    rng = np.random.RandomState(0)
    records, augs = [], []
    for i in range(B):
        joints = np.ones((K, 3))
        joints[:, 0], joints[:, 1] = rng.rand(K) * 200 + 220, rng.rand(K) * 300 + 90
        vis = np.ones((K, 3))
        vis[:, 2] = 0
        near = np.ones((M, K, 3))
        near[:, :, 0], near[:, :, 1] = rng.rand(M, K) * 300 + 170, rng.rand(M, K) * 360 + 60
        center, scale = np.array([320.0, 240.0], np.float32), np.array([1.35, 1.8], np.float32)
        records.append({"image": torch.from_numpy(rng.randint(0, 256, (IMG_H, IMG_W, 3)).astype(np.uint8)).to(dev),
                        "joints_3d": joints, "joints_3d_vis": vis, "near_joints": near.reshape(-1), "center": center,
                        "scale": scale})
        augs.append((center, scale * np.float32(0.8 + 0.4 * rng.rand()), float(rng.randn() * 30) if i % 5 < 3 else 0, bool(i % 2)))

    def new(seed):
        return pipe(records, augs, seed=seed)[0]

    def hand(seed):
        J = np.stack([r["joints_3d"] for r in records])
        area = []
        for cj in J:                                           # JointsDataset.py:204-210 per record
            xs, ys = cj[:, 0][np.nonzero(cj[:, 0])], cj[:, 1][np.nonzero(cj[:, 1])]
            area.append((np.max(xs) - np.min(xs)) * (np.max(ys) - np.min(ys)))
        near = np.stack([np.asarray(r["near_joints"]).reshape(-1, K, 3) for r in records])
        synth = synthesize_pose_batch("crowdpose", J, J, near, area, [0] * B, seed, device=dev).cpu().numpy()
        geos = [pipe.geometry(dict(r, cond_joints=synth[i], cond_joints_vis=r["joints_3d_vis"]), augs[i])
                for i, r in enumerate(records)]
        return pipe.render([r["image"] for r in records], geos)[0]

    fn = new if a.path == "new" else hand
    host, batch = [], []
    for it in range(WARMUP + BATCHES):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x = fn(1000 + it)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if it >= WARMUP:
            host.append((t1 - t0) * 1e3)
            batch.append((t2 - t0) * 1e3)
    assert x.shape == (B, 6, 384, 288) and float(x[:, 3:].abs().amax(dim=(1, 2, 3)).min()) > 0

    def stat(v):
        return [round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)]

    res = {"path": a.path, "tree": os.path.relpath(a.tree), "shape": {"B": B, "K": K, "M": M, "image_size": [288, 384]},
           "batches": BATCHES, "unit": "ms per batch: median [min, max]", "host_ms": stat(host), "batch_ms": stat(batch),
           "samples_per_s": round(B / statistics.median(batch) * 1e3, 1), "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
