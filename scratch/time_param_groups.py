"""The optimizer step alone on the arena of the benchmark configuration (BUCTD-CoAM-W48, bench.py train_c4): the plain
buctd_adam_step against the grouped kernel (csrc/optim_groups.hip) with one group over everything and with the
head / trunk / no-decay split of engine.groups_by_name.  One process; five rounds, the three variants in turn in every round,
20 launches between two events per variant and round; the figure of a variant is its best round, per launch.  Writes
profiles/param_groups_timing.json (or the path given as the first argument).

    python scratch/time_param_groups.py [out.json]
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from buctd_amd import _C, engine, models, ops  # noqa: E402

ROUNDS, LAUNCHES = 5, 20
HYPER = (2e-3, 0.9, 0.999, 1e-8)


def events_ms(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "param_groups_timing.json")
    dev = torch.device("cuda:0")
    cfg = bench.coam_w48_cfg(32)
    net = models.pose_hrnet_coam.get_pose_net(cfg, is_train=True).to(dev)
    flat = engine.FlatParams(net)
    flat.grad.normal_(generator=torch.Generator(device=dev).manual_seed(0))
    for p in flat.params:
        p.grad = flat(p)
    m, v = torch.zeros_like(flat.flat), torch.zeros_like(flat.flat)
    lr, b1, b2, eps = HYPER
    split = engine.groups_by_name(net, [("final_layer", {"lr": 10 * lr, "weight_decay": 1e-2}), ("", {"weight_decay": 1e-2})],
                                  no_decay_for_norm_and_bias=True)
    variants = {}

    def plain():
        ops.adam_step(flat.flat, flat.grad, m, v, lr, b1, b2, eps, 10)
    variants["plain_adam_step"] = (plain, {"elements": flat.numel})
    for name, groups, decoupled in (("grouped_one_group", [{"params": flat.params}], False), ("grouped_split", split, True)):
        opt = engine.FusedAdam(flat, lr=lr, groups=groups, decoupled_weight_decay=decoupled)
        live = opt._live_set()
        table = (_C.AdamGroup * len(opt.param_groups))()
        for t, g in zip(table, opt.param_groups):
            t.lr, t.beta1, t.beta2, t.eps, t.weight_decay = g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"]
            t.decoupled, t.step = int(g["decoupled_weight_decay"]), 10
        del opt.exp_avg, opt.exp_avg_sq

        def run(live=live, table=table):
            ops.adam_step_groups(flat.flat, flat.grad, m, v, live.table, table, 1.0, None)
        variants[name] = (run, {"groups": len(groups), "group_sizes": [len(g["params"]) for g in groups],
                                "chunks": live.table.numel() // 16, "spans": len(live.runs),
                                "elements": sum(e - s for s, e in live.runs)})
    for fn, _ in variants.values():                 # warm-up: code objects, the arena's pages
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, (fn, _) in variants.items():
            rounds[k].append(events_ms(fn, LAUNCHES))
    result = {"device": torch.cuda.get_device_name(0), "arena_elements": flat.numel, "parameters": len(flat.params),
              "rounds": ROUNDS, "launches_per_round": LAUNCHES, "bytes_per_element": 28, "variants": {}}
    for k, (_, info) in variants.items():
        best = min(rounds[k])
        result["variants"][k] = dict(info, ms_per_launch_min=best, ms_per_launch_rounds=rounds[k],
                                     spread_ms=max(rounds[k]) - min(rounds[k]), gb_per_s=28e-6 * info["elements"] / best)
    result["plain_round_to_round_spread_ms"] = result["variants"]["plain_adam_step"]["spread_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
