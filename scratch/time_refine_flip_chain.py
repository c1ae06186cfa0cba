"""Times a 3-pass IterativeRefiner.run with the flip test on the MI355X (sibling of time_refine_chain.py; same records,
same clock): TransPose-H-A6 256x192 (BASELINE C5), seeded random weights, images resident on the device.

  settings   host_flip          host chain, flip_test=True
             device_flip        device chain, flip_test=True
             device_flip_graph  device chain, flip_test=True, engine.ForwardGraph around the network (2B-row signature)
             device_noflip      device chain without the flip test - also what --tree DIR (another checkout with its own
                                built library, e.g. the parent commit, which has no flip keyword) can run
  sizes      1, 4 and 32 persons per call

Per size: WARMUP calls of each setting, then ROUNDS rounds that alternate the settings, RUNS calls each.  call time = until
the device is idle (torch.cuda.synchronize), host time = until run() returns; medians over all timed calls with min and
max, and the largest difference between two round medians of the same setting (the spread a difference has to exceed).
Two trees cannot share a process: compare them by alternating whole invocations and read the spread between invocations
of the same tree.

    python scratch/time_refine_flip_chain.py [--tree DIR] [--settings a,b] [--sizes 1,4,32] --out FILE.json"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROUNDS, RUNS, WARMUP, PASSES = 4, 5, 3, 3
IMG_H, IMG_W = 480, 640
COCO_FLIP_PAIRS = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]
SETTINGS = {"host_flip": (False, True, False), "device_flip": (True, True, False),
            "device_flip_graph": (True, True, True), "device_noflip": (True, False, False)}   # on_device, flip, graph


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--settings", default=",".join(SETTINGS))
    ap.add_argument("--sizes", default="1,4,32")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import bench
    from buctd_amd import engine, models
    from buctd_amd.dataset.pipeline import DeviceSamplePipeline, IterativeRefiner
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    dev = torch.device("cuda:0")
    settings = a.settings.split(",")
    cfg = bench.transpose_a6_cfg(32)
    torch.manual_seed(1234)
    net = models.transpose_h.get_pose_net(cfg, is_train=False).to(dev).eval()
    K = cfg.MODEL.NUM_JOINTS
    pipe = DeviceSamplePipeline(cfg, COCO_FLIP_PAIRS, range(8), bench.COCO_COLORS, is_train=False)
    points = []
    for B in (int(v) for v in a.sizes.split(",")):
        rng = np.random.RandomState(B)
        image = torch.from_numpy(rng.randint(0, 256, (IMG_H, IMG_W, 3)).astype(np.uint8)).to(dev)
        records = []
        for i in range(B):
            cond = np.ones((K, 3))
            cond[:, 0], cond[:, 1] = rng.rand(K) * 200 + 220, rng.rand(K) * 300 + 90
            records.append({"image": image, "joints_3d": np.zeros((K, 3)), "joints_3d_vis": np.ones((K, 3)),
                            "cond_joints": cond, "cond_joints_vis": np.ones((K, 3)), "score": 0.9,
                            "center": np.array([320.0 + i, 240.0], np.float32), "scale": np.array([1.35, 1.8], np.float32)})
        fns = {}
        for s in settings:
            on_device, flip, graph = SETTINGS[s]
            model = engine.ForwardGraph(net, warmup=1, autoselect=False) if graph else net
            kw = dict(flip_test=True, shift_heatmap=True) if flip else {}
            fns[s] = IterativeRefiner(cfg, model, pipe, on_device=on_device, **kw)
        call, host = {s: [[] for _ in range(ROUNDS)] for s in settings}, {s: [] for s in settings}
        for s in settings:
            for _ in range(WARMUP):
                last = fns[s].run(records, PASSES)
            assert len(last) == PASSES and last[-1]["preds"].shape == (B, K, 3)
        for r in range(ROUNDS):
            for s in settings:
                for _ in range(RUNS):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fns[s].run(records, PASSES)
                    t1 = time.perf_counter()
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                    host[s].append((t1 - t0) * 1e3)
                    call[s][r].append((t2 - t0) * 1e3)
        for s in settings:
            every = [v for r in call[s] for v in r]
            med = statistics.median(every)
            rounds = [statistics.median(r) for r in call[s]]
            pt = {"net": "transpose_h_a6", "persons": B, "setting": s, "tree": os.path.relpath(a.tree),
                  "call_ms": [round(med, 3), round(min(every), 3), round(max(every), 3)],
                  "round_spread_ms": round(max(rounds) - min(rounds), 3),
                  "host_ms": [round(statistics.median(host[s]), 3), round(min(host[s]), 3), round(max(host[s]), 3)],
                  "persons_per_s": round(B / med * 1e3, 1)}
            points.append(pt)
            print(json.dumps(pt), flush=True)
    res = {"what": "3-pass IterativeRefiner.run with the flip test, images resident on the device",
           "unit": "ms per call: median [min, max]", "rounds": ROUNDS, "runs_per_round": RUNS, "warmup": WARMUP,
           "device": torch.cuda.get_device_name(0), "points": points}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
