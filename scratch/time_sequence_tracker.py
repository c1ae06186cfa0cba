"""Times SequenceTracker.run on the MI355X: frames/s of the device loop against the host loop, frames resident on the device.

  network    preNet HRNet-W32 256x192, seeded random weights, eager and under engine.ForwardGraph
  sizes      M = 8 and M = 16 track slots; T = 12 frames of 480 x 640; M / 2 persons detected in frame 0, one more in
             frames 3 and 6 (what the network makes of them decides the deaths: the same on both paths)
  paths      device = SequenceTracker(on_device=True), host = the same class with on_device=False, on this tree

Per point: WARMUP calls of each path, then ROUNDS rounds that alternate the paths, RUNS calls each.  call time = until
the device is idle (torch.cuda.synchronize); medians over all timed calls with min and max, and the largest difference
between two round medians of the same path (the spread a difference has to exceed).

    python scratch/time_sequence_tracker.py [--sizes 8,16] --out FILE.json"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROUNDS, RUNS, WARMUP, FRAMES = 3, 3, 2, 12
IMG_H, IMG_W = 480, 640


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8,16")
    ap.add_argument("--wraps", default="eager,forward_graph")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    from buctd_amd import engine, models
    from buctd_amd.dataset.pipeline import DeviceSamplePipeline, SequenceTracker
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    dev = torch.device("cuda:0")
    cfg = bench.prenet_cfg(16, 32, (192, 256))
    torch.manual_seed(1234)
    net = models.pose_hrnet.get_pose_net(cfg, is_train=False).to(dev).eval()
    K = cfg.MODEL.NUM_JOINTS
    pipe = DeviceSamplePipeline(cfg, [], range(8), bench.COCO_COLORS, is_train=False)
    sigmas = None if K == 17 else np.full(K, 0.07)
    points = []
    for M in (int(v) for v in a.sizes.split(",")):
        rng = np.random.RandomState(M)
        frames = [torch.from_numpy(rng.randint(0, 256, (IMG_H, IMG_W, 3)).astype(np.uint8)).to(dev) for _ in range(FRAMES)]

        def person(i):
            pose = np.ones((K, 3)) * 0.8
            cx, cy = 60 + (i % 8) * 70, 120 + (i // 8) * 220
            pose[:, 0], pose[:, 1] = cx + rng.rand(K) * 40 - 20, cy + rng.rand(K) * 120 - 60
            return pose
        dets = [np.zeros((0, K, 3)) for _ in range(FRAMES)]
        dets[0] = np.stack([person(i) for i in range(M // 2)])
        dets[3], dets[6] = person(M // 2)[None], person(M // 2 + 1)[None]
        for wrap in a.wraps.split(","):
            model = net if wrap == "eager" else engine.ForwardGraph(net, warmup=1, autoselect=False)
            fns = {"device": SequenceTracker(cfg, model, pipe, max_tracks=M, sigmas=sigmas, on_device=True),
                   "host": SequenceTracker(cfg, model, pipe, max_tracks=M, sigmas=sigmas)}
            call = {p: [[] for _ in range(ROUNDS)] for p in fns}
            live = {}
            for path, fn in fns.items():
                for _ in range(WARMUP):
                    last = fn.run(frames, dets)
                assert len(last) == FRAMES and last[-1]["preds"].shape == (M, K, 3)
                live[path] = [int((f["ids"] >= 0).sum()) for f in last]
            for r in range(ROUNDS):
                for path, fn in fns.items():
                    for _ in range(RUNS):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fn.run(frames, dets)
                        torch.cuda.synchronize()
                        call[path][r].append((time.perf_counter() - t0) * 1e3)
            for path in fns:
                every = [v for r in call[path] for v in r]
                med = statistics.median(every)
                rounds = [statistics.median(r) for r in call[path]]
                pt = {"net": "hrnet_w32_prenet_256x192", "slots": M, "frames": FRAMES, "wrap": wrap, "path": path,
                      "live_per_frame": live[path], "call_ms": [round(med, 3), round(min(every), 3), round(max(every), 3)],
                      "round_spread_ms": round(max(rounds) - min(rounds), 3), "frames_per_s": round(FRAMES / med * 1e3, 1)}
                points.append(pt)
                print(json.dumps(pt), flush=True)
    res = {"what": "SequenceTracker.run over 12 frames, frames resident on the device; host = on_device=False on the same tree",
           "unit": "ms per call: median [min, max]", "rounds": ROUNDS, "runs_per_round": RUNS, "warmup": WARMUP,
           "device": torch.cuda.get_device_name(0), "points": points}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
