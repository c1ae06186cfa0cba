"""Eager engine against engine.StepGraph(..., fresh_dropout_masks=True) for the dropout models: ms per step, images/s and host
enqueue time per step, interleaved A/B rounds on one box.  Models: C4 (CoAM-W48 384x288, bench.py train_c4) and TransPose-H-A6
256x192 training.  Both paths train (fresh masks, the same seed stream); each round times `--steps` steps of each path.
    python scratch/step_graph_dropout_probe.py --model c4 --batch 8 [--rounds 3 --steps 20 --streams single]"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="c4", choices=["c4", "transpose_a6"])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--streams", default="single")
    args = ap.parse_args()
    from buctd_amd import engine, models, ops
    from buctd_amd.core.loss import JointsMSELoss
    rank, world, device = engine.init_distributed()
    ops.set_conv_math("bf16x6")
    bench.first_touch(device)
    if args.model == "c4":
        cfg, module = bench.coam_w48_cfg(args.batch), "pose_hrnet_coam"
    else:
        cfg, module = bench.transpose_a6_cfg(args.batch), "transpose_h"
    torch.manual_seed(1234)
    ops.manual_seed(1234)
    net = getattr(models, module).get_pose_net(cfg, is_train=True).to(device)
    model = engine.DataParallel(net)
    optimizer = engine.get_optimizer(cfg, model)
    model.flatten()
    criterion = JointsMSELoss(cfg.LOSS.USE_TARGET_WEIGHT)
    x, target, weight = bench.synthetic_batch(cfg, args.batch, device, seed=100)
    model.train()

    def eager():
        out = model(x)
        loss = criterion(out, target, weight)
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        return loss

    gs = engine.StepGraph(model, criterion, optimizer, warmup=0, streams=args.streams, fresh_dropout_masks=True)

    def graphed():
        return gs(x, target, weight)[1]

    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = 0.0
        for _ in range(n):
            a = time.perf_counter()
            loss = fn()
            host += time.perf_counter() - a
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / n, 1e3 * host / n, float(loss.detach())

    for _ in range(3):
        eager()
    drawn = ops.seeds_drawn()
    eager()
    per_step = ops.seeds_drawn() - drawn
    t0 = time.perf_counter()
    graphed()
    torch.cuda.synchronize()
    print(f"{args.model} batch {args.batch}: {per_step} dropout draws per step; capture + first replay "
          f"{time.perf_counter() - t0:.2f} s", flush=True)
    res = {"eager": [], "graph": []}
    for _ in range(args.rounds):
        for name, fn in (("eager", eager), ("graph", graphed)):
            res[name].append(timed(fn, args.steps))
    for name, rows in res.items():
        ms = [r[0] for r in rows]
        med, host = statistics.median(ms), statistics.median(r[1] for r in rows)
        print(f"{args.model} batch {args.batch} {name}: median {med:.2f} ms/step = {args.batch / med * 1e3:.1f} img/s "
              f"(spread {100 * (max(ms) - min(ms)) / med:.1f} %, n={len(ms)}), host {host:.2f} ms/step, "
              f"last loss {rows[-1][2]:.6f}", flush=True)
    e, g = statistics.median(r[0] for r in res["eager"]), statistics.median(r[0] for r in res["graph"])
    print(f"{args.model} batch {args.batch}: graph / eager throughput {e / g:.3f}", flush=True)


if __name__ == "__main__":
    main()
