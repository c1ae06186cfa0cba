"""Wall clock of a generative-sampling train batch with the scalar geometry on the device (geometry_on_device=True)
against the host geometry() of the same tree and of another tree (the parent commit), with and without use_bu_bbox records
(which send the host path to its fallback): batch 32, 384 x 288, K = 14, M = 2 neighbours, colored condition, 480 x 640
images resident on the device; the pipeline makes its own augmentation draws.  One process per row:

    python scratch/time_geometry_pipeline.py --mode on|off [--bu] [--tree DIR] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

B, K, M, IMG_H, IMG_W, WARMUP, BATCHES = 32, 14, 2, 480, 640, 8, 40
FLIP_PAIRS = [[0, 1], [2, 3], [4, 5], [6, 7], [8, 9], [10, 11]]
COLORS = [[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [255, 0, 255], [0, 255, 255], [128, 255, 0], [255, 128, 0],
          [0, 128, 255], [128, 0, 255], [255, 0, 128], [0, 255, 128], [200, 200, 200], [120, 120, 120]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["on", "off"], required=True)
    ap.add_argument("--bu", action="store_true", help="every second record has use_bu_bbox=True")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    from buctd_amd.config import cfg as base
    from buctd_amd.dataset.pipeline import DeviceSamplePipeline
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    dev = torch.device("cuda:0")
    c = base.clone()
    c.defrost()
    c.MODEL.NUM_JOINTS, c.MODEL.IMAGE_SIZE, c.MODEL.HEATMAP_SIZE, c.MODEL.SIGMA = K, [288, 384], [72, 96], 3
    c.MODEL.CONDITIONAL_TOPDOWN, c.DATASET.COLORED, c.DATASET.DATASET = True, True, "crowdpose"
    c.DATASET.SYNTHESIS_POSE = True
    c.freeze()
    kw = {"geometry_on_device": True} if a.mode == "on" else {}
    pipe = DeviceSamplePipeline(c, FLIP_PAIRS, range(8), COLORS, is_train=True, seed=0, **kw)
    rng = np.random.RandomState(0)
    records = []
    for i in range(B):
        joints = np.ones((K, 3))
        joints[:, 0], joints[:, 1] = rng.rand(K) * 200 + 220, rng.rand(K) * 300 + 90
        vis = np.ones((K, 3))
        vis[:, 2] = 0
        near = np.ones((M, K, 3))
        near[:, :, 0], near[:, :, 1] = rng.rand(M, K) * 300 + 170, rng.rand(M, K) * 360 + 60
        records.append({"image": torch.from_numpy(rng.randint(0, 256, (IMG_H, IMG_W, 3)).astype(np.uint8)).to(dev),
                        "joints_3d": joints, "joints_3d_vis": vis, "near_joints": near.reshape(-1),
                        "center": np.array([320.0, 240.0], np.float32), "scale": np.array([1.35, 1.8], np.float32),
                        "use_bu_bbox": bool(a.bu and i % 2 == 0)})
    host, batch = [], []
    for it in range(WARMUP + BATCHES):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x = pipe(records, seed=1000 + it)[0]
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if it >= WARMUP:
            host.append((t1 - t0) * 1e3)
            batch.append((t2 - t0) * 1e3)
    assert x.shape == (B, 6, 384, 288) and float(x[:, 3:].abs().amax(dim=(1, 2, 3)).min()) > 0

    def stat(v):
        return [round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)]

    res = {"mode": a.mode, "use_bu_bbox": bool(a.bu), "tree": os.path.relpath(a.tree),
           "shape": {"B": B, "K": K, "M": M, "image_size": [288, 384]}, "batches": BATCHES,
           "unit": "ms per batch: median [min, max]", "host_ms": stat(host), "batch_ms": stat(batch),
           "samples_per_s": round(B / statistics.median(batch) * 1e3, 1), "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
