"""Times a 3-pass IterativeRefiner.run on the MI355X: persons/s with the images resident on the device.

  networks   TransPose-H-A6 256x192 (BASELINE C5) and preNet HRNet-W32 256x192, seeded random weights
  sizes      1, 4 and 32 persons per call
  wrapping   the eager engine, and engine.ForwardGraph around the network
  paths      device = IterativeRefiner(on_device=True), host = the default path; --tree DIR --paths host times the host
             path of another checkout (with its own built library), e.g. the parent commit

Per point: WARMUP calls of each path, then ROUNDS rounds that alternate the paths, RUNS calls each.  call time = until
the device is idle (torch.cuda.synchronize), host time = until run() returns; medians over all timed calls with min and
max, and the largest difference between two round medians of the same path (the spread a difference has to exceed).

    python scratch/time_refine_chain.py [--tree DIR] [--paths device,host] [--sizes 1,4,32] --out FILE.json"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROUNDS, RUNS, WARMUP, PASSES = 4, 5, 4, 3
IMG_H, IMG_W = 480, 640


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--paths", default="device,host")
    ap.add_argument("--sizes", default="1,4,32")
    ap.add_argument("--nets", default="transpose_h_a6,hrnet_w32")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import bench
    from buctd_amd import engine, models
    from buctd_amd.dataset.pipeline import DeviceSamplePipeline, IterativeRefiner
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    dev = torch.device("cuda:0")
    paths = a.paths.split(",")
    nets = {"transpose_h_a6": (lambda b: bench.transpose_a6_cfg(b), "transpose_h"),
            "hrnet_w32": (lambda b: bench.prenet_cfg(b, 32, (192, 256)), "pose_hrnet")}
    points = []
    for net_name in a.nets.split(","):
        make_cfg, module = nets[net_name]
        cfg = make_cfg(32)
        torch.manual_seed(1234)
        net = getattr(models, module).get_pose_net(cfg, is_train=False).to(dev).eval()
        K = cfg.MODEL.NUM_JOINTS
        pipe = DeviceSamplePipeline(cfg, [], range(8), bench.COCO_COLORS, is_train=False)
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
            for wrap in ("eager", "forward_graph"):
                model = net if wrap == "eager" else engine.ForwardGraph(net, warmup=1, autoselect=False)
                fns = {}
                for path in paths:
                    kw = {"on_device": True} if path == "device" else {}
                    fns[path] = IterativeRefiner(cfg, model, pipe, **kw)
                call, host = {p: [[] for _ in range(ROUNDS)] for p in paths}, {p: [] for p in paths}
                for path in paths:
                    for _ in range(WARMUP):
                        last = fns[path].run(records, PASSES)
                    assert len(last) == PASSES and last[-1]["preds"].shape == (B, K, 3)
                for r in range(ROUNDS):
                    for path in paths:
                        for _ in range(RUNS):
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            fns[path].run(records, PASSES)
                            t1 = time.perf_counter()
                            torch.cuda.synchronize()
                            t2 = time.perf_counter()
                            host[path].append((t1 - t0) * 1e3)
                            call[path][r].append((t2 - t0) * 1e3)
                for path in paths:
                    every = [v for r in call[path] for v in r]
                    med = statistics.median(every)
                    rounds = [statistics.median(r) for r in call[path]]
                    pt = {"net": net_name, "persons": B, "wrap": wrap, "path": path, "tree": os.path.relpath(a.tree),
                          "call_ms": [round(med, 3), round(min(every), 3), round(max(every), 3)],
                          "round_spread_ms": round(max(rounds) - min(rounds), 3),
                          "host_ms": [round(statistics.median(host[path]), 3), round(min(host[path]), 3), round(max(host[path]), 3)],
                          "persons_per_s": round(B / med * 1e3, 1)}
                    points.append(pt)
                    print(json.dumps(pt), flush=True)
    res = {"what": "3-pass IterativeRefiner.run, images resident on the device", "unit": "ms per call: median [min, max]",
           "rounds": ROUNDS, "runs_per_round": RUNS, "warmup": WARMUP, "device": torch.cuda.get_device_name(0), "points": points}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
