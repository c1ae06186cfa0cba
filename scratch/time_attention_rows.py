"""attention_rows at T = 3072, d = 112, h = 1, B = 2: R = 17 and the full map, next to the materialised route
(buctd_matmul logits + buctd_softmax_dropout_fwd, p = 0, as ops.PositionAttention runs them); alternating, medians.
A timed call is the host op as a user calls it: attention_rows allocates its output inside the window (torch's caching
allocator hands the same block back - 75 MB for the full map); the materialised route writes into one buffer made once."""
import json, math, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from buctd_amd import ops

dev = torch.device("cuda:0")
B, T, d, h = 2, 3072, 112, 1
g = torch.Generator().manual_seed(0)
qk = (torch.randn(B, T, 2 * d, generator=g) * 1.2).to(dev)
rows = torch.randint(0, T, (B, 17), generator=g, dtype=torch.int32).to(dev)
S = torch.empty((B, h, T, T), dtype=torch.float32, device=dev)
scale = 1.0 / math.sqrt(d)

def rows17():
    return ops.attention_rows(qk, rows, h)
def full():
    return ops.attention_rows(qk, None, h)
def materialised():
    ops.matmul(qk, qk, S, batch=B, M=T, N=T, K=d, a_layout=0, b_layout=0, lda=2 * d, ldb=2 * d, ldc=T,
               stride_a=T * 2 * d, stride_b=T * 2 * d, stride_c=h * T * T, a_off=0, b_off=d, c_off=0)
    return ops.softmax_dropout_fwd(S, T, scale, 0.0, ops.next_seed())[0]

fns = {"rows17": rows17, "full": full, "materialised": materialised}
a = full(); b_ = materialised()
print("full vs materialised rel", ((a.double() - b_.view(B, T, T).double()).norm() / b_.double().norm()).item())
for f in fns.values():
    for _ in range(5):
        f()
torch.cuda.synchronize()
N, REP = 40, 7
res = {k: [] for k in fns}
for rep in range(REP):
    for name, f in fns.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(N):
            f()
        e1.record()
        torch.cuda.synchronize()
        res[name].append(e0.elapsed_time(e1) / N * 1e3)
out = {k: {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)} for k, v in res.items()}
out["shape"] = {"B": B, "T": T, "d": d, "h": h, "calls_per_window": N, "windows": REP}
print(json.dumps(out))
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "attention_rows_timing.json"), "w") as f:
    f.write(json.dumps(out, indent=1) + "\n")
