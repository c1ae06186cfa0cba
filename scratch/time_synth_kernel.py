"""buctd_synthesize_pose alone on one build of libbuctd_hip.so: does reading the ladder thresholds from
buctd_synth_tables cost anything against the literals of the parent commit?  One library per process - the package loads
its library with RTLD_GLOBAL, so a second build in the same process would run the first one's kernels - and the caller
alternates processes:

    python scratch/time_synth_kernel.py --lib buctd_amd/lib/libbuctd_hip.so --dump this.npy --out this.json
    python scratch/time_synth_kernel.py --lib /path/to/parent/libbuctd_hip.so --dump parent.npy --out parent.json
    cmp this.npy parent.npy

B = 32 persons, K = 14 (crowdpose tables), M = 2 neighbours: the headline batch.  5 rounds of 200 launches between two
device events, each after 20 warm-up launches; --dump keeps the poses of seed 4242 for the bit comparison.  A library that
takes the shorter struct of the parent reads only its own prefix of the tables."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True)
    ap.add_argument("--out", default=None)
    ap.add_argument("--dump", default=None)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    from oracle import pose_synthesis as P
    from buctd_amd.dataset.pose_synthesis import make_tables
    dev = torch.device("cuda:0")
    fn = C.CDLL(os.path.abspath(a.lib)).buctd_synthesize_pose
    fn.restype = C.c_int
    joints, est, near, area = P.make_scene("crowdpose", 7)
    B, K, M = 32, 14, 2
    J = torch.from_numpy(np.stack([joints] * B)).to(dev)
    E = torch.from_numpy(np.stack([est] * B)).to(dev)
    N = torch.from_numpy(np.stack([near] * B)).to(dev)
    J[4, 6:, 2] = 0                                           # few annotated joints: the ladders' other rows
    A = torch.full((B,), area, dtype=torch.float64, device=dev)
    ov = torch.zeros(B, dtype=torch.int32, device=dev)
    ov[3], ov[4] = 3, 1
    tables = make_tables("crowdpose", K)
    out = torch.empty((B, K, 3), dtype=torch.float64, device=dev)

    def launch(seed):
        rc = fn(C.byref(tables), *(C.c_void_p(t.data_ptr()) for t in (J, E, N, A, ov)), B, K, M, C.c_ulonglong(seed),
                C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc

    launch(4242)
    torch.cuda.synchronize()
    if a.dump:
        np.save(a.dump, out.cpu().numpy())
    us = []
    for _ in range(a.rounds):
        for i in range(20):
            launch(i)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for i in range(a.launches):
            launch(100 + i)
        t1.record()
        torch.cuda.synchronize()
        us.append(1000.0 * t0.elapsed_time(t1) / a.launches)
    line = {"what": "buctd_synthesize_pose, us per launch, B 32 K 14 M 2", "lib": a.lib, "median": float(np.median(us)),
            "rounds": [round(x, 2) for x in us]}
    print(json.dumps(line))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(line, f, indent=1)


if __name__ == "__main__":
    main()
