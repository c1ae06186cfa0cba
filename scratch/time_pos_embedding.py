"""usage: time_pos_embedding.py OUT.json : buctd_batch_sum alone at the TransPose-H-A6 256x192 sizes, device events around
many launches; 'rotating' walks 8 inputs (8 x 44 MB at batch 32: more than the 256 MB Infinity Cache), 'resident' one"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from buctd_amd import _C  # noqa: E402

out_path = sys.argv[1]
dev = torch.device("cuda:0")
lib = _C.lib()
N = 3072 * 112
res = []
for batch in (32, 2):
    xs = [torch.randn(batch, N, device=dev) for _ in range(8)]
    out = torch.zeros(N, device=dev)
    ref = xs[0].double().sum(0)
    _C.check(lib.buctd_batch_sum(xs[0].data_ptr(), batch, N, out.data_ptr(), 0, _C.stream_ptr()), "batch_sum")
    err = float((out.double() - ref).abs().max())
    for mode, bufs in (("rotating", xs), ("resident", xs[:1])):
        iters = 400
        for i in range(40):
            lib.buctd_batch_sum(bufs[i % len(bufs)].data_ptr(), batch, N, out.data_ptr(), 1, _C.stream_ptr())
        torch.cuda.synchronize()
        best = None
        for rep in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(iters):
                lib.buctd_batch_sum(bufs[i % len(bufs)].data_ptr(), batch, N, out.data_ptr(), 1, _C.stream_ptr())
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / iters
            best = us if best is None else min(best, us)
        nbytes = 4 * N * (batch + 2)          # rows read, out read (accumulate) and written
        res.append({"kernel": "buctd_batch_sum", "batch": batch, "n": N, "accumulate": 1, "inputs": mode,
                    "us_per_launch_back_to_back": best, "bytes": nbytes, "GB_per_s": nbytes / best / 1e3,
                    "max_abs_err_vs_fp64": err, "load_1min": os.getloadavg()[0]})
        print(json.dumps(res[-1]), flush=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
