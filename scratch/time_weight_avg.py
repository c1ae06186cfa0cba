"""engine.WeightAverage on the arena of the benchmark configuration (BUCTD-CoAM-W48, bench.py train_c4): update() with
buffers="live" (one buctd_ema_update over the arena) and with buffers="average" (plus one buctd_ema_update_tensors over the
BatchNorm statistics), and applied() enter + exit (two buctd_swap over the arena, two refreshes of the prepared filter images;
with buffers="average" one more swap per buffer on either side).  One train step at batch 2 runs first, so that the prepared
images an optimizer step refreshes exist.  One process; 3 warm-up rounds, then ROUNDS rounds with the variants in turn;
update(): LAUNCHES calls between two events per round, applied(): one enter + exit between two events per round.  Reported
per variant: the median round, min, max, and for update() the achieved rate over its own traffic of 12 bytes per element.
Writes profiles/weight_avg_timing.json (or the path given as the first argument).

    python scratch/time_weight_avg.py [out.json]
"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from buctd_amd import engine, models  # noqa: E402
from buctd_amd.core.loss import JointsMSELoss  # noqa: E402

ROUNDS, LAUNCHES, WARMUP = 9, 20, 3


def events_ms(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "weight_avg_timing.json")
    dev = torch.device("cuda:0")
    cfg = bench.coam_w48_cfg(2)
    torch.manual_seed(1234)
    net = models.pose_hrnet_coam.get_pose_net(cfg, is_train=True).to(dev)
    model = engine.DataParallel(net)
    opt = engine.get_optimizer(cfg, model)
    model.flatten()
    model.train()
    x, target, weight = bench.synthetic_batch(cfg, 2, dev, seed=100)
    loss = JointsMSELoss(cfg.LOSS.USE_TARGET_WEIGHT)(model(x), target, weight)
    opt.zero_grad()
    loss.backward()
    opt.step()
    opt.zero_grad()
    del loss
    flat = opt.flat
    live = engine.WeightAverage(flat, 0.9998)
    both = engine.WeightAverage(flat, 0.9998, buffers="average")

    def enter_exit(avg):
        with avg.applied():
            pass
    variants = {
        "update_live": (live.update, LAUNCHES),
        "update_average_buffers": (both.update, LAUNCHES),
        "applied_enter_exit_live": (lambda: enter_exit(live), 1),
        "applied_enter_exit_average_buffers": (lambda: enter_exit(both), 1),
    }
    for _ in range(WARMUP):
        for fn, n in variants.values():
            events_ms(fn, n)
    torch.cuda.synchronize()
    rounds = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, (fn, n) in variants.items():
            rounds[k].append(events_ms(fn, n))
    buffer_elements = sum(v.numel() for v in both._buffer_views())
    result = {"device": torch.cuda.get_device_name(0), "arena_elements": flat.numel, "arena_mb": flat.numel * 4 / 2 ** 20,
              "parameters": len(flat.params), "averaged_buffers": len(both._names), "buffer_elements": buffer_elements,
              "rounds": ROUNDS, "warmup_rounds": WARMUP, "launches_per_round_update": LAUNCHES, "variants": {}}
    for k, ms in rounds.items():
        med = statistics.median(ms)
        entry = {"ms_median": med, "ms_min": min(ms), "ms_max": max(ms), "ms_rounds": ms}
        if k.startswith("update"):
            elements = flat.numel + (buffer_elements if k.endswith("buffers") else 0)
            entry.update(bytes_per_element=12, tb_per_s_median=12e-9 * elements / med, tb_per_s_best=12e-9 * elements / min(ms))
        else:
            entry.update(swap_bytes_per_element=16, swap_traffic_only_tb_per_s=2 * 16e-9 * flat.numel / med)
        result["variants"][k] = entry
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
