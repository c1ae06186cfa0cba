"""usage: time_grad_sumsq.py OUT.json : buctd_grad_sumsq (+ buctd_grad_clip_coef) alone on a gradient arena of the CoAM-W48
network's size (462 MB), one run over the whole arena; device events around each launch, two arenas in turn
(each alone is larger than the 256 MB Infinity Cache).  Reports the median of the launches after a warm-up and their spread,
and the plain and the _dscale Adam step on the same arena for comparison."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from buctd_amd import ops  # noqa: E402

out_path = sys.argv[1]
assert torch.cuda.is_available(), "a timing needs the device"
dev = torch.device("cuda:0")
N = 462 * 1000 * 1000 // 4 // 4 * 4
runs = [(0, N)]
arenas = [torch.randn(N, device=dev) for _ in range(2)]
sumsq = torch.zeros(1, dtype=torch.float64, device=dev)
ws = torch.zeros(ops.grad_sumsq_workspace(runs) // 8, dtype=torch.float64, device=dev)
coef, norm = torch.ones(1, device=dev), torch.zeros(1, device=dev)
ops.grad_sumsq(arenas[0], runs, sumsq, ws)
ref = float(arenas[0].double().square().sum())
rel = abs(sumsq.item() - ref) / ref
p, m, v = (torch.zeros(N, device=dev) for _ in range(3))


def reduce_only(i):
    ops.grad_sumsq(arenas[i % 2], runs, sumsq, ws)


def reduce_and_finalize(i):
    ops.grad_sumsq(arenas[i % 2], runs, sumsq, ws)
    ops.grad_clip_coef(sumsq, 1.0, 1e30, coef, norm)


def adam_plain(i):
    ops.adam_step(p, arenas[i % 2], m, v, 1e-3, 0.9, 0.999, 1e-8, i + 1, 1.0)


def adam_dscale(i):
    ops.adam_step(p, arenas[i % 2], m, v, 1e-3, 0.9, 0.999, 1e-8, i + 1, 1.0, coef)


res = []
for name, fn, nbytes in (("buctd_grad_sumsq", reduce_only, 4 * N + 16 * ws.numel()),
                         ("buctd_grad_sumsq + buctd_grad_clip_coef", reduce_and_finalize, 4 * N + 16 * ws.numel()),
                         ("buctd_adam_step", adam_plain, 7 * 4 * N),
                         ("buctd_adam_step_dscale", adam_dscale, 7 * 4 * N)):
    for i in range(10):
        fn(i)
    torch.cuda.synchronize()
    times = []
    for i in range(60):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(i)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    times.sort()
    med = statistics.median(times)
    res.append({"what": name, "elements": N, "bytes": nbytes, "launches": len(times), "us_median": med, "us_min": times[0],
                "us_p10": times[len(times) // 10], "us_p90": times[len(times) * 9 // 10], "us_max": times[-1],
                "GB_per_s_at_median": nbytes / med / 1e3, "rel_err_vs_torch_fp64": rel, "load_1min": os.getloadavg()[0]})
    print(json.dumps(res[-1]), flush=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
