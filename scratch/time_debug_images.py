"""Cost of one debug picture dump (utils/vis.py) at B = 32, 384 x 288, K = 17, heat-maps 96 x 72: save_debug_images with
the three flags set (wall clock around a device synchronize, median / min / max of 7 calls after a warm-up) and the two
render calls alone (events).  Writes profiles/debug_images_timing.json (or the path given as the first argument).

    python scratch/time_debug_images.py [out.json]
"""
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from buctd_amd.config import cfg as base_cfg  # noqa: E402
from buctd_amd.utils import vis  # noqa: E402

B, H, W, K, Hh, Wh, CALLS = 32, 384, 288, 17, 96, 72, 7


def events_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "samples": xs}


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "debug_images_timing.json")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, 3, H, W, generator=g).to(dev)
    target = torch.rand(B, K, Hh, Wh, generator=g).to(dev)
    output = torch.randn(B, K, Hh, Wh, generator=g).to(dev)
    joints = torch.rand(B, K, 3, generator=g) * torch.tensor([W, H, 0.0])
    meta = {"joints": joints, "joints_vis": torch.ones(B, K, 3)}
    pred = (joints[:, :, :2] + 2.0).numpy()
    cfg = base_cfg.clone()
    cfg.defrost()
    cfg.DEBUG.DEBUG = cfg.DEBUG.SAVE_BATCH_IMAGES_PRED = cfg.DEBUG.SAVE_HEATMAPS_GT = cfg.DEBUG.SAVE_HEATMAPS_PRED = True

    with tempfile.TemporaryDirectory() as tmp:
        def dump():
            vis.save_debug_images(cfg, x, meta, target, pred, output, os.path.join(tmp, "train_0"))
            torch.cuda.synchronize()
        dump()
        wall = []
        for _ in range(CALLS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dump()
            wall.append((time.perf_counter() - t0) * 1e3)
        sizes = {os.path.relpath(os.path.join(d, f), tmp): os.path.getsize(os.path.join(d, f))
                 for d, _, fs in os.walk(tmp) for f in fs}

    heat = lambda: vis.render_batch_heatmaps(x, output, bgr=True)
    grid = lambda: vis.render_batch_image_with_joints(x, pred, meta["joints_vis"], meta, bgr=True)
    heat(), grid()
    torch.cuda.synchronize()
    heat_ms = [events_ms(heat) for _ in range(CALLS)]
    grid_ms = [events_ms(grid) for _ in range(CALLS)]
    pictures = {"heatmap_grid": list(heat().shape), "joint_grid": list(grid().shape)}
    # what the reference copies to the host per dump (fp32 input, target, output) against the three uint8 pictures
    ref_bytes = 4 * (x.numel() + target.numel() + output.numel())
    our_bytes = 2 * int(np.prod(pictures["heatmap_grid"])) + int(np.prod(pictures["joint_grid"]))
    result = {"shape": {"B": B, "H": H, "W": W, "K": K, "Hh": Hh, "Wh": Wh}, "device": torch.cuda.get_device_name(0),
              "calls": CALLS, "save_debug_images_wall_ms": summary(wall), "render_batch_heatmaps_event_ms": summary(heat_ms),
              "render_batch_image_with_joints_event_ms": summary(grid_ms), "pictures": pictures, "png_bytes": sizes,
              "host_copy_bytes": {"reference_fp32": ref_bytes, "uint8_pictures": our_bytes}}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
