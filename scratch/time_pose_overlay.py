"""Timing of the pose overlay at a user's size: 1920 x 1080, 20 persons, 'coco', plain.
    python scratch/time_pose_overlay.py [out.json]
The kernel alone by device events over 200 launches of one call's argument struct (7 samples), and the whole draw_poses
call - table building, one upload, launch - by the host clock around a device synchronise (200 calls)."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from buctd_amd.utils import vis

dev = torch.device('cuda:0')
H, W, P = 1080, 1920, 20
rng = np.random.default_rng(0)
canvas = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).to(dev)
# persons of about 300 x 600 pixels spread over the picture
centre = np.stack([rng.uniform(200, W - 200, P), rng.uniform(320, H - 320, P)], axis=-1)
poses = (centre[:, None, :] + rng.uniform(-1, 1, (P, 17, 2)) * np.array([150, 300])).astype(np.float32)
poses_dev = torch.from_numpy(poses).to(dev)

kernel_ms = []
real_lib = vis.lib


class Proxy:
    """re-launches the call's argument struct while its tables are alive: the kernel alone, by device events"""
    def __getattr__(self, name):
        return getattr(real_lib(), name)

    def buctd_vis_pose_overlay(self, args, stream):
        fn = real_lib().buctd_vis_pose_overlay
        for _ in range(20):
            fn(args, stream)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(200):
            rc = fn(args, stream)
        e1.record()
        torch.cuda.synchronize()
        kernel_ms.append(e0.elapsed_time(e1) / 200)
        return rc


def wall(fn, n):
    out = []
    for _ in range(n):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return out


call = lambda: vis.draw_poses(canvas, poses_dev, skeleton='coco')
wall(call, 10)
calls = wall(call, 200)
vis.lib = lambda: Proxy()
for _ in range(7):
    call()
vis.lib = real_lib
tiles = -(-H // 16) * -(-W // 64)
res = {"shape": {"H": H, "W": W, "persons": P, "skeleton": "coco", "style": "plain", "thickness": 2, "radius": 3,
                 "primitives": P * (17 + 18), "tiles": tiles},
       "device": torch.cuda.get_device_name(0),
       "kernel_event_ms_mean_of_200_launches": {"median": statistics.median(kernel_ms), "min": min(kernel_ms),
                                                "max": max(kernel_ms), "samples": kernel_ms},
       "draw_poses_wall_ms_with_synchronise": {"median": statistics.median(calls), "min": min(calls), "max": max(calls),
                                               "p90": sorted(calls)[180]}}
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], 'w'), indent=1)
print(json.dumps({k: v for k, v in res.items() if k != 'shape'})[:600])
